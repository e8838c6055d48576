"""CPU checks of the loss kinds (st_plan_set_loss_kinds, StyleTransfer.content_loss / style_loss, --content-loss /
--style-loss): the header declares the entries and the library exports them, the up-front validation (`_resolve_loss_kinds`)
accepts and refuses what it should, stylize() refuses the same before any device work, and the CLI flags reach the
attributes - no GPU needed."""
import os
import re
import types

import pytest

from conftest import REPO

NEW_ENTRIES = ['st_plan_set_loss_kinds', 'st_plan_loss_kinds']


def _lib():
    from style_transfer import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip, _hip.load_library(require_gpu=False)


def test_header_declares_and_library_exports_the_entries():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'st_amd.h')).read(), flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert hip.CONTENT_LOSSES == ('mse', 'scaled_mse') and hip.STYLE_LOSSES == ('w2', 'gram')
    assert (hip.Plan.content_loss, hip.Plan.style_loss) == ('mse', 'w2')


@pytest.mark.parametrize('world', [1, 2, 8])
def test_the_defaults_pass_for_any_world_size(world):
    from style_transfer.style_transfer import _resolve_loss_kinds
    assert _resolve_loss_kinds('mse', 'w2', world) == ('mse', 'w2')


def test_every_kind_passes_on_one_rank():
    from style_transfer.style_transfer import _resolve_loss_kinds
    for content in ('mse', 'scaled_mse'):
        for style in ('w2', 'gram'):
            assert _resolve_loss_kinds(content, style, 1) == (content, style)
            assert _resolve_loss_kinds(content, style) == (content, style)


@pytest.mark.parametrize('content, style, choices', [
    ('l1', 'w2', ['mse', 'scaled_mse']),
    ('mse', 'gatys', ['w2', 'gram']),
    ('MSE', 'w2', ['mse', 'scaled_mse']),
    (None, 'w2', ['mse', 'scaled_mse']),
    ('mse', 1, ['w2', 'gram']),
])
def test_an_unknown_name_is_refused_with_the_choices(content, style, choices):
    from style_transfer.style_transfer import _resolve_loss_kinds
    with pytest.raises(ValueError) as err:
        _resolve_loss_kinds(content, style, 1)
    for name in choices:
        assert repr(name) in str(err.value), str(err.value)


@pytest.mark.parametrize('content, style', [('scaled_mse', 'w2'), ('mse', 'gram'), ('scaled_mse', 'gram')])
def test_a_non_default_kind_is_refused_on_several_ranks(content, style):
    from style_transfer.style_transfer import _resolve_loss_kinds
    with pytest.raises(ValueError, match='strips'):
        _resolve_loss_kinds(content, style, world=2)


def _bare_style_transfer(devices):
    """A StyleTransfer without the constructor's device work (tests/test_taps_cpu.py builds one the same way)."""
    import torch
    from style_transfer import StyleTransfer
    st = StyleTransfer.__new__(StyleTransfer)
    st.devices = [torch.device(d) for d in devices]
    st._job = None
    st.content_layers, st.style_layers = [22], [1, 6, 11, 20, 29]
    st.style_weights = [w / 341 for w in (256, 64, 16, 4, 1)]
    return st


def test_stylize_refuses_before_any_device_work():
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    assert (st.content_loss, st.style_loss) == ('mse', 'w2')             # the class's defaults
    st.style_loss = 'gram'
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st.style_loss, st.content_loss = 'w2', 'scaled_mse'
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st = _bare_style_transfer(['cuda:0'])
    st.style_loss = 'gatys'
    with pytest.raises(ValueError, match=r"'w2', 'gram'"):
        st.stylize(None, [None])
    st.style_loss, st.content_loss = 'gram', 'huber'
    with pytest.raises(ValueError, match=r"'mse', 'scaled_mse'"):
        st.stylize(None, [None])


def test_stylize_keeps_its_signature():
    from style_transfer import StyleTransfer
    assert 'content_loss' not in StyleTransfer.stylize.__kwdefaults__ and 'style_loss' not in StyleTransfer.stylize.__kwdefaults__


def test_cli_flags_parse_and_land_on_the_attributes():
    from style_transfer import cli
    parser = cli.build_parser()
    args = parser.parse_args(['content.png', 'style.png'])
    assert (args.content_loss, args.style_loss) == ('mse', 'w2')
    st = cli.apply_loss_kinds(types.SimpleNamespace(), args)
    assert (st.content_loss, st.style_loss) == ('mse', 'w2')
    args = parser.parse_args(['content.png', 'style.png', '--content-loss', 'scaled_mse', '--style-loss', 'gram'])
    st = cli.apply_loss_kinds(_bare_style_transfer(['cuda:0']), args)
    assert (st.content_loss, st.style_loss) == ('scaled_mse', 'gram')
    for bad in (['--style-loss', 'gatys'], ['--content-loss', 'l1']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])
    # the flags are the parser's alone: stylize() is not handed them
    from style_transfer import StyleTransfer
    assert not {'content_loss', 'style_loss'} & set(StyleTransfer.stylize.__kwdefaults__)

"""CPU checks of the spatial weight maps for the content and TV terms (st_plan_set_content_mask / st_plan_content_mask /
st_plan_set_tv_mask / st_plan_tv_mask, StyleTransfer.content_mask / tv_mask, --content-mask / --tv-mask): the header declares
the entries and the library exports them, the up-front validation (`_resolve_weight_maps`) accepts and refuses what it should,
stylize() refuses the same before any device work, and the CLI options reach the attributes - no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from test_loss_kinds_cpu import _bare_style_transfer, _lib
from test_style_mask_cpu import _pil, _ramp

NEW_ENTRIES = ['st_plan_set_content_mask', 'st_plan_content_mask', 'st_plan_set_tv_mask', 'st_plan_tv_mask']
ATTRIBUTES = ['content_mask', 'tv_mask']


def _resolve(content_mask=None, tv_mask=None, world=1):
    from style_transfer.style_transfer import _resolve_weight_maps
    return _resolve_weight_maps(content_mask, tv_mask, world)


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert lib.st_abi_version() == 2
    for name in ('set_content_mask', 'content_mask_level', 'set_tv_mask', 'tv_mask'):
        assert callable(getattr(hip.Plan, name, None)), name
    # the semantics are fixed in the header: both formulas and the normaliser's rule
    comment = ' '.join(header[:header.index('int st_plan_set_content_mask(')].rsplit('/*', 1)[1].replace('*', ' ').split())
    for phrase in ('avg_pool2d', 'element count', 'replicate-padded', 'two end points', 'equal bits', 'strip plan'):
        assert phrase in comment, f'include/st_amd.h, st_plan_set_content_mask: {phrase!r} is not documented'


def test_no_map_is_the_default_for_any_world_size():
    from style_transfer import StyleTransfer
    assert StyleTransfer.content_mask is None and StyleTransfer.tv_mask is None       # class attributes
    for world in (1, 2, 8):
        assert _resolve(world=world) == (None, None)


def test_the_accepted_forms():
    ramp = _ramp(40, 48)
    for given in (ramp, torch.from_numpy(ramp), ramp.astype(np.float64), ramp.tolist()):
        (image, divisor), none = _resolve(given)
        assert image.mode == 'F' and image.size == (48, 40) and divisor == 1.0 and none is None
        assert np.array_equal(np.asarray(image), ramp)
    none, (image, divisor) = _resolve(None, _pil(ramp).convert('RGB'))
    assert none is None and image.mode == 'L' and image.size == (48, 40) and divisor == 255.0
    content, tv = _resolve(_pil(ramp), np.ones((3, 5), np.float32))
    assert content[0].mode == 'L' and tv[0].mode == 'F' and tv[0].size == (5, 3)


@pytest.mark.parametrize('attribute', ATTRIBUTES)
@pytest.mark.parametrize('bad', [np.ones((3, 4, 4), np.float32), np.ones(16, np.float32), np.float32(0.5), 'mask.png'],
                         ids=['3-d', '1-d', '0-d', 'path'])
def test_a_wrong_number_of_dimensions_is_refused(attribute, bad):
    with pytest.raises(ValueError, match=attribute):
        _resolve(**{attribute: bad})


@pytest.mark.parametrize('attribute', ATTRIBUTES)
@pytest.mark.parametrize('bad', [1.5, -0.25, float('nan'), float('inf')])
def test_values_outside_the_unit_interval_are_refused(attribute, bad):
    mask = _ramp(16, 16)
    mask[3, 5] = bad
    with pytest.raises(ValueError, match=attribute):
        _resolve(**{attribute: mask})
    with pytest.raises(ValueError, match=attribute):
        _resolve(**{attribute: torch.from_numpy(mask)})


@pytest.mark.parametrize('attribute', ATTRIBUTES)
def test_an_all_zero_map_is_refused(attribute):
    for zero in (np.zeros((16, 16), np.float32), torch.zeros((16, 16)), _pil(np.zeros((16, 16)))):
        with pytest.raises(ValueError, match=f'{attribute}.*zero') as info:
            _resolve(**{attribute: zero})
        assert 'style' not in str(info.value)


@pytest.mark.parametrize('attribute', ATTRIBUTES)
def test_a_map_is_refused_on_several_ranks(attribute):
    assert _resolve(**{attribute: _ramp(16, 16)}, world=1)
    with pytest.raises(ValueError, match=f'{attribute}.*strips'):
        _resolve(**{attribute: _ramp(16, 16)}, world=2)


@pytest.mark.parametrize('attribute', ATTRIBUTES)
def test_stylize_refuses_before_any_device_work(attribute):
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    assert st.content_mask is None and st.tv_mask is None
    setattr(st, attribute, _ramp(16, 16))
    with pytest.raises(ValueError, match=f'{attribute}.*strips'):
        st.stylize(None, [None])
    st = _bare_style_transfer(['cuda:0'])
    for bad in (np.zeros((16, 16), np.float32), np.full((16, 16), 1.5, np.float32), np.ones((2, 16, 16), np.float32)):
        setattr(st, attribute, bad)
        with pytest.raises(ValueError, match=attribute):
            st.stylize(None, [None])


def test_stylize_keeps_its_signature():
    from style_transfer import StyleTransfer
    assert not set(ATTRIBUTES) & set(StyleTransfer.stylize.__kwdefaults__)
    assert len(StyleTransfer.stylize.__kwdefaults__) == 14


def test_cli_options_parse_and_land_on_the_attributes(tmp_path):
    import types
    from style_transfer import cli
    parser = cli.build_parser()
    args = parser.parse_args(['content.png', 'a.png'])
    assert args.content_mask is None and args.tv_mask is None
    st = cli.apply_weight_maps(types.SimpleNamespace(), args)
    assert st.content_mask is None and st.tv_mask is None
    content_path, tv_path = str(tmp_path / 'content_mask.png'), str(tmp_path / 'tv_mask.png')
    _pil(_ramp(20, 30)).save(content_path)
    _pil(_ramp(24, 36)).save(tv_path)
    args = parser.parse_args(['content.png', 'a.png', '--content-mask', content_path, '--tv-mask', tv_path])
    assert args.content_mask == content_path and args.tv_mask == tv_path
    st = cli.apply_weight_maps(_bare_style_transfer(['cuda:0']), args)
    assert st.content_mask.mode == 'L' and st.content_mask.size == (30, 20)
    assert st.tv_mask.mode == 'L' and st.tv_mask.size == (36, 24)
    content, tv = _resolve(st.content_mask, st.tv_mask)
    assert content[1] == 255.0 and tv[1] == 255.0
    for bad in (['--content-mask'], ['--tv-mask'], ['--content-mask', content_path, 'extra', '--content-mask']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])
    for option in ('--content-mask', '--tv-mask'):                      # a file that cannot be read
        with pytest.raises(SystemExit):
            cli.apply_weight_maps(_bare_style_transfer(['cuda:0']), parser.parse_args(
                ['content.png', 'a.png', option, str(tmp_path / 'missing.png')]))

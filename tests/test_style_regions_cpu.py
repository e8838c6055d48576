"""CPU checks of the style regions (st_plan_set_style_regions and its four companions, StyleTransfer.style_regions /
style_image_regions / style_region_weights, --style-regions / --style-image-regions / --style-region-weights): the header
declares the entries and the library exports them, the up-front validation (`_resolve_style_regions`) accepts and refuses what
it should, stylize() refuses the same before any device work, and the CLI options parse - no GPU needed."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO
from test_loss_kinds_cpu import _bare_style_transfer, _lib
from test_style_mask_cpu import _pil, _ramp

NEW_ENTRIES = ['st_plan_set_style_regions', 'st_plan_style_region', 'st_plan_set_region_style_target',
               'st_plan_set_region_weights', 'st_plan_region_terms']


def _resolve(style_regions=None, style_image_regions=None, style_region_weights=None, n=2, style_weights=None, style_mask=None,
             world=1):
    from style_transfer.style_transfer import _resolve_style_regions
    return _resolve_style_regions(style_regions, style_image_regions, style_region_weights, n, style_weights, style_mask, world)


def _two():
    ramp = _ramp(40, 48)
    return [ramp, 1 - ramp]


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert lib.st_abi_version() == 2 and re.search(r'#define\s+ST_AMD_ABI_VERSION\s+2\b', header)
    for name in ('set_style_regions', 'style_region_level', 'set_region_style_target', 'set_region_weights', 'region_term_losses'):
        assert hasattr(hip.Plan, name), name


def test_no_regions_is_the_default_for_any_world_size():
    from style_transfer import StyleTransfer
    assert StyleTransfer.style_regions is None and StyleTransfer.style_image_regions is None
    assert StyleTransfer.style_region_weights is None
    for world in (1, 2, 8):
        assert _resolve(world=world) is None


def test_the_accepted_forms():
    ramp = _ramp(40, 48)
    regions, image_regions, weights = _resolve(_two(), [1, 0])
    assert len(regions) == 2 and image_regions == [1, 0] and weights is None
    assert all(image.mode == 'F' and image.size == (48, 40) and divisor == 1.0 for image, divisor in regions)
    assert np.array_equal(np.asarray(regions[1][0]), 1 - ramp)
    # every form of a mask, several images in a region, numpy integers as indices, weights used as given
    regions, image_regions, weights = _resolve((_pil(ramp), torch.from_numpy(ramp), ramp.tolist()), np.array([0, 2, 1, 0]),
                                               (2, 0, 0.5), n=4, style_weights=[2, 1, 1, -1])
    assert [image.mode for image, _ in regions] == ['L', 'F', 'F'] and image_regions == [0, 2, 1, 0] and weights == [2.0, 0.0, 0.5]
    # one region, and four
    assert _resolve([ramp], [0], n=1)[1] == [0]
    assert len(_resolve([ramp] * 4, [0, 1, 2, 3], n=4)[0]) == 4
    # overlapping masks that do not sum to 1 are fine
    assert _resolve([ramp, ramp], [0, 1]) is not None


@pytest.mark.parametrize('kwargs, message', [
    (dict(style_regions=_two()), 'style_image_regions'),                                             # required with regions
    (dict(style_regions=_two(), style_image_regions=[0]), 'style_image_regions'),                  # a wrong length
    (dict(style_regions=_two(), style_image_regions=[0, 1, 1]), 'style_image_regions'),
    (dict(style_regions=_two(), style_image_regions=[0, 2]), r'style_image_regions\[1\].*out of range'),
    (dict(style_regions=_two(), style_image_regions=[-1, 1]), r'style_image_regions\[0\].*out of range'),
    (dict(style_regions=_two(), style_image_regions=[0.5, 1]), 'style_image_regions'),
    (dict(style_regions=_two(), style_image_regions=[0, 0]), 'style_image_regions.*region 1 has no style image'),
    (dict(style_regions=_two(), style_image_regions=[0, 1, 1], n=3, style_weights=[1, 1, -1]), 'style_image_regions.*region 1.*sum to 0'),
    (dict(style_regions=[_ramp(8, 8)] * 5, style_image_regions=[0, 1, 2, 3, 4], n=5), 'style_regions: 5 regions'),
    (dict(style_regions=[], style_image_regions=[]), 'style_regions: 0 regions'),
    (dict(style_regions=_ramp(8, 8), style_image_regions=[0, 0]), 'style_regions'),              # a bare mask is not a list of masks
    (dict(style_regions=_two(), style_image_regions=[0, 1], style_mask=_ramp(40, 48)), 'style_mask together with style_regions'),
    (dict(style_regions=_two(), style_image_regions=[0, 1], world=2), 'style_regions.*strips'),
    (dict(style_regions=[_ramp(8, 8), np.zeros((8, 8), np.float32)], style_image_regions=[0, 1]), r'style_regions\[1\].*zero'),
    (dict(style_regions=[np.full((8, 8), 1.5, np.float32)], style_image_regions=[0, 0]), r'style_regions\[0\]'),
    (dict(style_regions=[np.ones((2, 8, 8), np.float32)], style_image_regions=[0, 0]), r'style_regions\[0\]'),
    (dict(style_regions=_two(), style_image_regions=[0, 1], style_region_weights=[1]), 'style_region_weights'),
    (dict(style_regions=_two(), style_image_regions=[0, 1], style_region_weights=[1, -1]), 'style_region_weights'),
    (dict(style_regions=_two(), style_image_regions=[0, 1], style_region_weights=[0, 0]), 'style_region_weights'),
    (dict(style_regions=_two(), style_image_regions=[0, 1], style_region_weights=[1, float('nan')]), 'style_region_weights'),
    (dict(style_regions=_two(), style_image_regions=[0, 1], style_region_weights=0.5), 'style_region_weights'),
    (dict(style_image_regions=[0, 1]), 'without style_regions'),
    (dict(style_region_weights=[1, 1]), 'without style_regions'),
])
def test_what_is_refused(kwargs, message):
    with pytest.raises(ValueError, match=message):
        _resolve(**kwargs)


def test_stylize_refuses_before_any_device_work():
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    st.style_regions, st.style_image_regions = _two(), [0, 1]
    with pytest.raises(ValueError, match='style_regions.*strips'):
        st.stylize(None, [None, None])
    st = _bare_style_transfer(['cuda:0'])
    st.style_regions = _two()
    with pytest.raises(ValueError, match='style_image_regions'):
        st.stylize(None, [None, None])
    st.style_image_regions = [0, 0]
    with pytest.raises(ValueError, match='region 1 has no style image'):
        st.stylize(None, [None, None])
    st.style_image_regions = [0, 1]
    with pytest.raises(ValueError, match='sum to 0'):
        st.stylize(None, [None, None], style_weights=[1, 0])
    st.style_mask = _ramp(40, 48)
    with pytest.raises(ValueError, match='style_mask together with style_regions'):
        st.stylize(None, [None, None])
    st.style_mask, st.style_region_weights = None, [1, 2, 3]
    with pytest.raises(ValueError, match='style_region_weights'):
        st.stylize(None, [None, None])


def test_stylize_keeps_its_signature():
    from style_transfer import StyleTransfer
    assert not {'style_regions', 'style_image_regions', 'style_region_weights'} & set(StyleTransfer.stylize.__kwdefaults__)
    assert len(StyleTransfer.stylize.__kwdefaults__) == 14


def test_cli_options_parse_and_land_on_the_attributes(tmp_path):
    from style_transfer import cli
    parser = cli.build_parser()
    args = parser.parse_args(['content.png', 'a.png', 'b.png'])
    assert args.style_regions is None and args.style_image_regions is None and args.style_region_weights is None
    st = cli.apply_style_masks(types.SimpleNamespace(), args)
    assert st.style_regions is None and st.style_image_regions is None and st.style_region_weights is None
    sky, ground = str(tmp_path / 'sky.png'), str(tmp_path / 'ground.png')
    _pil(_ramp(20, 30)).save(sky)
    _pil(1 - _ramp(20, 30)).save(ground)
    args = parser.parse_args(['content.png', 'a.png', 'b.png', '--style-regions', sky, ground, '--style-image-regions', '1', '0',
                              '--style-region-weights', '0.75', '0.25'])
    assert args.style_regions == [sky, ground] and args.style_image_regions == [1, 0] and args.style_region_weights == [0.75, 0.25]
    st = cli.apply_style_masks(_bare_style_transfer(['cuda:0']), args)
    assert [m.mode for m in st.style_regions] == ['L', 'L'] and st.style_regions[1].size == (30, 20)
    assert st.style_image_regions == [1, 0] and st.style_region_weights == [0.75, 0.25]
    regions, image_regions, weights = _resolve(st.style_regions, st.style_image_regions, st.style_region_weights)
    assert len(regions) == 2 and image_regions == [1, 0] and weights == [0.75, 0.25]
    for bad in (['--style-regions'], ['--style-image-regions', 'sky'], ['--style-region-weights', 'half'], ['--style-image-regions']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])
    with pytest.raises(SystemExit):       # a file that cannot be read
        cli.apply_style_masks(_bare_style_transfer(['cuda:0']),
                              parser.parse_args(['content.png', 'a.png', '--style-regions', str(tmp_path / 'missing.png')]))

"""CPU checks of the spatial style masks (st_plan_set_style_mask / st_plan_style_mask, StyleTransfer.style_mask /
style_image_masks, --style-mask / --style-image-masks): the header declares the entries and the library exports them, the
up-front validation (`_resolve_style_masks`) accepts and refuses what it should, stylize() refuses the same before any device
work, the masks are brought to a scale's size as documented, and the CLI options parse - no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from test_loss_kinds_cpu import _bare_style_transfer, _lib

NEW_ENTRIES = ['st_plan_set_style_mask', 'st_plan_style_mask']


def _resolve(style_mask=None, style_image_masks=None, n=1, world=1):
    from style_transfer.style_transfer import _resolve_style_masks
    return _resolve_style_masks(style_mask, style_image_masks, n, world)


def _ramp(h, w):
    x = np.arange(w) / (w - 1)
    y = np.arange(h) / (h - 1)
    return (np.clip(2 * (x - 0.25), 0, 1)[None, :] * (0.5 + 0.5 * y)[:, None]).astype(np.float32)


def _pil(values):
    from PIL import Image
    return Image.fromarray(np.uint8(np.round(values * 255)), 'L')


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert lib.st_abi_version() == 2 and re.search(r'#define\s+ST_AMD_ABI_VERSION\s+2\b', header)
    for name in ('set_style_mask', 'style_mask_level'):
        assert hasattr(hip.Plan, name), name


def test_the_ramp_masks_level_sums():
    """The semantics' own numbers: level k + 1 = avg_pool2d(level k, 2) at floor sizes; the ramp at 40 x 48."""
    level = torch.from_numpy(_ramp(40, 48))
    for size, want in (((40, 48), 720), ((20, 24), 180), ((10, 12), 45), ((5, 6), 11.25), ((2, 3), 2.096)):
        assert tuple(level.shape) == size
        assert abs(float(level.double().sum()) - want) <= 1e-3 * want, (size, float(level.double().sum()))
        level = torch.nn.functional.avg_pool2d(level[None, None], 2)[0, 0]


def test_no_mask_is_the_default_for_any_world_size():
    from style_transfer import StyleTransfer
    assert StyleTransfer.style_mask is None and StyleTransfer.style_image_masks is None       # class attributes
    for world in (1, 2, 8):
        assert _resolve(world=world) == (None, [None])
        assert _resolve(None, [None, None], n=2, world=world) == (None, [None, None])


def test_the_accepted_forms():
    ramp = _ramp(40, 48)
    for given in (ramp, torch.from_numpy(ramp), ramp.astype(np.float64), ramp.tolist()):
        (image, divisor), per_image = _resolve(given)
        assert image.mode == 'F' and image.size == (48, 40) and divisor == 1.0 and per_image == [None]
        assert np.array_equal(np.asarray(image), ramp)
    (image, divisor), _ = _resolve(_pil(ramp).convert('RGB'))
    assert image.mode == 'L' and image.size == (48, 40) and divisor == 255.0
    output, per_image = _resolve(None, [None, ramp, _pil(ramp)], n=3)
    assert output is None and per_image[0] is None and per_image[1][0].mode == 'F' and per_image[2][0].mode == 'L'
    assert _resolve(np.ones((3, 5), np.float32), (np.ones((2, 2)),))[1][0][1] == 1.0


def test_a_mask_at_a_scales_size():
    """A PIL image: convert('L').resize((w, h), BILINEAR) / 255 in fp32; an array: the same resize of an 'F' image."""
    from PIL import Image
    from style_transfer.style_transfer import _sized_mask
    ramp = _ramp(48, 64)
    pil = _pil(ramp)
    got = _sized_mask(_resolve(pil)[0], 45, 34)
    want = np.asarray(pil.convert('L').resize((45, 34), Image.BILINEAR), dtype=np.float32) / np.float32(255)
    assert got.dtype == torch.float32 and tuple(got.shape) == (34, 45) and np.array_equal(got.numpy(), want)
    got = _sized_mask(_resolve(ramp)[0], 45, 34)
    want = np.asarray(Image.fromarray(ramp, mode='F').resize((45, 34), Image.BILINEAR), dtype=np.float32)
    assert tuple(got.shape) == (34, 45) and np.allclose(got.numpy(), want, rtol=0, atol=1e-6)
    assert float(got.min()) >= 0 and float(got.max()) <= 1
    assert np.array_equal(_sized_mask(_resolve(ramp)[0], 64, 48).numpy(), ramp)


@pytest.mark.parametrize('kwargs, attribute', [
    (dict(style_image_masks=[None, None]), 'style_image_masks'),
    (dict(style_image_masks=[]), 'style_image_masks'),
    (dict(style_image_masks=[None], n=2), 'style_image_masks'),
    (dict(style_image_masks=np.ones((4, 4), np.float32)), 'style_image_masks'),        # a bare mask is not a list of masks
    (dict(style_mask=np.ones((3, 4, 4), np.float32)), 'style_mask'),
    (dict(style_mask=np.ones(16, np.float32)), 'style_mask'),
    (dict(style_mask=np.float32(0.5)), 'style_mask'),
    (dict(style_image_masks=[np.ones((1, 4, 4))]), r'style_image_masks\[0\]'),
    (dict(style_mask='mask.png'), 'style_mask'),
])
def test_a_wrong_length_or_shape_is_refused(kwargs, attribute):
    with pytest.raises(ValueError, match=attribute):
        _resolve(**kwargs)


@pytest.mark.parametrize('bad', [1.5, -0.25, float('nan'), float('inf')])
def test_values_outside_the_unit_interval_are_refused(bad):
    mask = _ramp(16, 16)
    mask[3, 5] = bad
    with pytest.raises(ValueError, match='style_mask'):
        _resolve(mask)
    with pytest.raises(ValueError, match=r'style_image_masks\[1\]'):
        _resolve(None, [None, torch.from_numpy(mask)], n=2)


def test_an_all_zero_mask_is_refused():
    for zero in (np.zeros((16, 16), np.float32), torch.zeros((16, 16)), _pil(np.zeros((16, 16)))):
        with pytest.raises(ValueError, match='style_mask.*zero'):
            _resolve(zero)
        with pytest.raises(ValueError, match=r'style_image_masks\[0\].*zero'):
            _resolve(None, [zero])


@pytest.mark.parametrize('kwargs', [dict(style_mask=_ramp(16, 16)), dict(style_image_masks=[_ramp(16, 16)])])
def test_a_mask_is_refused_on_several_ranks(kwargs):
    assert _resolve(**kwargs, world=1)
    with pytest.raises(ValueError, match='strips'):
        _resolve(**kwargs, world=2)


def test_stylize_refuses_before_any_device_work():
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    assert st.style_mask is None and st.style_image_masks is None
    st.style_mask = _ramp(16, 16)
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st.style_mask, st.style_image_masks = None, [_pil(_ramp(16, 16))]
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st = _bare_style_transfer(['cuda:0'])
    st.style_image_masks = [None, None]
    with pytest.raises(ValueError, match='style_image_masks'):
        st.stylize(None, [None])
    st.style_image_masks, st.style_mask = None, np.zeros((16, 16), np.float32)
    with pytest.raises(ValueError, match='style_mask'):
        st.stylize(None, [None])
    st.style_mask = np.full((16, 16), 1.5, np.float32)
    with pytest.raises(ValueError, match='style_mask'):
        st.stylize(None, [None])
    st.style_mask = np.ones((2, 16, 16), np.float32)
    with pytest.raises(ValueError, match='style_mask'):
        st.stylize(None, [None])


def test_stylize_keeps_its_signature():
    from style_transfer import StyleTransfer
    assert not {'style_mask', 'style_image_masks'} & set(StyleTransfer.stylize.__kwdefaults__)
    assert len(StyleTransfer.stylize.__kwdefaults__) == 14


def test_cli_options_parse_and_land_on_the_attributes(tmp_path):
    import types
    from style_transfer import cli
    parser = cli.build_parser()
    args = parser.parse_args(['content.png', 'a.png', 'b.png'])
    assert args.style_mask is None and args.style_image_masks is None
    st = cli.apply_style_masks(types.SimpleNamespace(), args)
    assert st.style_mask is None and st.style_image_masks is None
    path = str(tmp_path / 'mask.png')
    _pil(_ramp(20, 30)).save(path)
    args = parser.parse_args(['content.png', 'a.png', 'b.png', '--style-mask', path, '--style-image-masks', 'none', path])
    assert args.style_mask == path and args.style_image_masks == ['none', path]
    st = cli.apply_style_masks(_bare_style_transfer(['cuda:0']), args)
    assert st.style_mask.mode == 'L' and st.style_mask.size == (30, 20)
    assert st.style_image_masks[0] is None and st.style_image_masks[1].size == (30, 20)
    assert _resolve(st.style_mask, st.style_image_masks, n=2)[1][0] is None
    for bad in (['--style-mask'], ['--style-image-masks'], ['--style-mask', path, 'extra', '--style-mask']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])
    # one entry per style image, and a file that cannot be read
    for argv in (['content.png', 'a.png', 'b.png', '--style-image-masks', path],
                 ['content.png', 'a.png', '--style-mask', str(tmp_path / 'missing.png')]):
        with pytest.raises(SystemExit):
            cli.apply_style_masks(_bare_style_transfer(['cuda:0']), parser.parse_args(argv))

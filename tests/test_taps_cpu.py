"""CPU checks of the configurable content / style layers: the header declares the new entries, the built library exports
them, the ctypes binding binds them, the switch that forces the general closure is not an environment switch, and
StyleTransfer's up-front validation (`_resolve_taps`) accepts and refuses what it should - no GPU needed."""
import os
import re

import pytest

from conftest import REPO

NEW_ENTRIES = ['st_plan_set_taps', 'st_plan_set_tap_weights', 'st_plan_set_content_target_at', 'st_plan_term_losses']
DEFAULT = ([22], [1, 6, 11, 20, 29])
CONFIGS = {                                   # the configurations of tests/test_taps_gpu.py
    'a': ([20], [1, 6, 11, 20, 29]),
    'b': ([22, 29], [1, 6, 11, 20, 29]),
    'c': ([22], [1, 6, 11, 20]),
    'd': ([18], [1, 13, 27]),
    'e': ([22], [3, 8, 17, 26]),
    'f': ([], [6]),
    'g': ([11], []),
}


def _header():
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _lib():
    from style_transfer import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip, _hip.load_library(require_gpu=False)


def test_header_declares_the_new_entries_and_keeps_the_abi_version():
    text = _header()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
    assert re.search(r'#define\s+ST_AMD_ABI_VERSION\s+2\b', text)


def test_library_exports_and_binding_binds_them():
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
        assert getattr(lib, name).argtypes is not None
    assert lib.st_abi_version() == 2


def test_the_forcing_switch_is_not_an_environment_switch():
    hip, lib = _lib()
    names = hip.env_switches()
    assert 'ST_GENERAL_TAPS' not in names and len(names) == 13
    hip.set_option('ST_GENERAL_TAPS', 1)          # ... it answers to st_set_option
    hip.set_option('ST_GENERAL_TAPS', None)


def test_taps_are_the_seventeen_the_trunk_keeps():
    hip, _ = _lib()
    import st_oracle as O
    want = sorted(idx for idx, op, _ in O.layer_program() if op in ('relu', 'pool'))
    assert list(hip.TAPS) == want and len(want) == 17
    assert (list(hip.DEFAULT_CONTENT_LAYERS), list(hip.DEFAULT_STYLE_LAYERS)) == (O.CONTENT_LAYERS, O.STYLE_LAYERS)


def test_resolve_taps_accepts_the_default_and_the_tested_configurations():
    from style_transfer.style_transfer import _resolve_taps
    weights = [w / 341 for w in (256, 64, 16, 4, 1)]
    assert _resolve_taps(*DEFAULT, weights) == (DEFAULT[0], DEFAULT[1], weights)
    assert _resolve_taps(*DEFAULT, weights, world=4) == (DEFAULT[0], DEFAULT[1], weights)      # strips run the default
    for content, style in CONFIGS.values():
        got = _resolve_taps(content, style, weights)
        # the pairs are zip(style_layers, style_weights), as the reference forms them (:451)
        assert got == (content, style[:5], weights[:len(style)])
    # a longer layer list than weights: zip() ends at the shorter one
    assert _resolve_taps([22], [1, 3, 6, 8, 11, 13], weights) == ([22], [1, 3, 6, 8, 11], weights)


@pytest.mark.parametrize('content, style, text', [
    ([2], [1, 6, 11, 20, 29], 'pre-ReLU'),                      # conv1_2's output: not a tap of the fused trunk
    ([22], [1, 6, 0, 20, 29], '17 taps'),
    ([22, 22], [1, 6, 11, 20, 29], 'twice'),
    ([22], [1, 6, 6], 'twice'),
    ([1, 3, 4, 6, 8, 9, 11, 13, 15, 17, 18, 20, 22, 24, 26, 27, 29], [1], 'at most 16'),
    ([], [], 'both empty'),
])
def test_resolve_taps_refuses(content, style, text):
    from style_transfer.style_transfer import _resolve_taps
    with pytest.raises(ValueError, match=text):
        _resolve_taps(content, style, [1.0] * 17)


def test_resolve_taps_refuses_other_layers_on_several_ranks():
    from style_transfer.style_transfer import _resolve_taps
    with pytest.raises(ValueError, match='strips'):
        _resolve_taps([20, 22], [1, 6, 11], [0.5, 0.3, 0.2], world=2)


def test_a_device_list_with_other_layers_fails_before_any_worker_starts():
    """stylize() validates first: two devices and a non-default layer set raise on the calling process, with no GPU touched
    (the constructor needs one, so the instance is made without it)."""
    from style_transfer import StyleTransfer
    import torch
    st = StyleTransfer.__new__(StyleTransfer)
    st.devices = [torch.device('cuda:0'), torch.device('cuda:1')]
    st._job = None
    st.content_layers, st.style_layers, st.style_weights = [20, 22], [1, 6, 11], [0.5, 0.3, 0.2]
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st.devices = st.devices[:1]
    st.content_layers = [2]
    with pytest.raises(ValueError, match='pre-ReLU'):
        st.stylize(None, [None])

"""CPU checks of the drop-in boundary: the C-ABI library loads and exports exactly the symbols that
include/st_amd.h declares (no compute calls - there is no GPU here), and the product path refuses to
run without a GPU instead of falling back."""
import os
import re

import pytest

from conftest import REPO


def _header_symbols():
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(st_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    from style_transfer import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load_library(require_gpu=False)
    declared = _header_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in st_amd.h but not exported by libst_amd.so'
    assert sorted(_hip.EXPORTED_SYMBOLS) == declared, 'ctypes binding and header disagree'
    assert lib.st_abi_version() == 2
    assert lib.st_compiled_arch() == b'gfx950'


def test_environment_switches_of_the_default_build_are_the_documented_ones():
    """a default library reads at most 15 ST_* switches from the environment, each documented in
    tools/README.md; every other switch answers to st_set_option only (or to a build with --experiments)."""
    from style_transfer import _hip
    names = _hip.env_switches()
    assert 0 < len(names) <= 15 and len(set(names)) == len(names)
    readme = open(os.path.join(REPO, 'tools', 'README.md')).read()
    section = readme.split('## Environment switches of the default build')[1].strip().split('\n\n')[0]
    documented = re.findall(r'`(ST_[A-Z0-9_]+)', section)
    assert sorted(set(documented)) == sorted(names), (sorted(set(documented)), sorted(names))
    # the library's own sources read the environment through option_env only (one place decides what is let through)
    csrc = os.path.join(REPO, 'style-transfer-pytorch_amd', 'csrc')
    for f in os.listdir(csrc):
        src = open(os.path.join(csrc, f)).read()
        for m in re.finditer(r'[^_a-z]getenv\(', src):
            line = src[:m.start()].count('\n') + 1
            assert f == 'st_api.hip' and 'return getenv(name);' in src.splitlines()[line - 1], f'{f}:{line} reads the environment directly'


def test_operand_bound_readout_is_documented():
    """st_plan_debug_read's what = 2 (tests/test_operand_bounds_gpu.py reads the 64 fp16x3 operand bounds through it): the
    header states the word map, the two sharing rules and when the words may be read; the binding refuses another count."""
    from style_transfer import _hip
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    comment = text[:text.index('int st_plan_debug_read(')].rsplit('/*', 1)[1]
    comment = ' '.join(comment.replace('*', ' ').split())
    for phrase in ('what = 2', 'count = 64', 'words 0 .. 12', 'words 16 .. 28', 'words 32 .. 35', 'words 48 .. 63', 'reads 0',
                   'a pooled map has no y word of its own', 'a convolution that feeds a pool has no g word of its own',
                   'st_plan_step and st_plan_lbfgs_step clear all 64 in their tail', 'what = 16 + i'):
        assert phrase in comment, f'include/st_amd.h, st_plan_debug_read: {phrase!r} is not documented'
    with pytest.raises(ValueError, match='64 operand bounds'):
        _hip.Plan.debug_read(None, 2, 63)
    assert 'bound word' in _hip.Plan.debug_read.__doc__


def test_default_build_has_no_experiment_kernels():
    """... and holds neither the persistent chain kernel nor the Winograd convolution (nm on the host library: kernel stubs)."""
    import subprocess
    from style_transfer import _hip
    lib = _hip.load_library(require_gpu=False)
    out = subprocess.run(['nm', '-C', _hip.LIB_PATH], capture_output=True, text=True).stdout
    has = ('ns_chain_kernel' in out, 'wino_conv_kernel' in out)
    if lib.st_has_experiments():
        assert all(has)
    else:
        assert not any(has), has


def test_no_cpu_fallback():
    import torch
    import style_transfer
    from style_transfer import _hip
    with pytest.raises(ValueError):
        style_transfer.StyleTransfer(devices=['cpu'], weights='synthetic')
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipLibraryError):
            _hip.load_library(require_gpu=True)


def test_package_does_not_import_the_oracle():
    pkg = os.path.join(REPO, 'style-transfer-pytorch_amd')
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(root, f)).read()
                assert 'st_oracle' not in src and 'oracle/' not in src, f'{f} references the oracle'

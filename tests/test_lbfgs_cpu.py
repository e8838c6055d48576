"""CPU check of the native L-BFGS step's surface: its entry points are declared in include/st_amd.h, exported by the library
and bound by the ctypes layer, and stylize()'s unsharded L-BFGS branch goes through them (no GPU here: no compute call)."""
import inspect
import os
import re

from conftest import REPO

LBFGS_SYMBOLS = ['st_lbfgs_info', 'st_lbfgs_reset', 'st_lbfgs_state_bytes', 'st_lbfgs_update', 'st_plan_lbfgs_step']


def test_lbfgs_entry_points_are_declared_exported_and_bound():
    from style_transfer import _hip
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(s for s in set(re.findall(r'\b(st_[a-z0-9_]+)\s*\(', text)) if 'lbfgs' in s)
    assert declared == LBFGS_SYMBOLS
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load_library(require_gpu=False)
    for name in LBFGS_SYMBOLS:
        assert hasattr(lib, name) and name in _hip.EXPORTED_SYMBOLS
    assert lib.st_abi_version() == 2                      # additions only
    # the state: a 4 KiB control block, the partial sums, 2 * 11 + 1 parameter-sized slots of 16-byte multiples
    small, large = lib.st_lbfgs_state_bytes(3 * 19 * 17), lib.st_lbfgs_state_bytes(3 * 64 * 64)
    assert large - small == 23 * 4 * (3 * 64 * 64 - 972) and small % 16 == 0
    assert lib.st_lbfgs_state_bytes(0) == 0
    for method in ('reset', 'step', 'update', 'info'):
        assert callable(getattr(_hip.LBFGS, method))


def test_stylize_runs_lbfgs_through_the_library():
    from style_transfer import style_transfer
    src = inspect.getsource(style_transfer.StyleTransfer.stylize)
    code = '\n'.join(line.split('#')[0] for line in src.splitlines())        # (comments cite torch's optimiser)
    assert '_hip.LBFGS(' in code and 'torch.optim' not in code and 'requires_grad_' not in code

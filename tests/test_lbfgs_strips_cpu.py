"""CPU check of the strip form of the native L-BFGS step: its entry points (named st_qn_*: tests/test_lbfgs_cpu.py pins the
set of names that contain `lbfgs`) are declared in include/st_amd.h, exported and bound; the strip state is the unsharded
layout plus a 16-byte multiple per rank; stylize()'s sharded L-BFGS branch goes through the library (no GPU: no compute)."""
import inspect
import os
import re

from conftest import REPO

QN_SYMBOLS = ['st_plan_qn_strip_step', 'st_qn_strip_apply', 'st_qn_strip_dots', 'st_qn_strip_state_bytes']


def _library():
    from style_transfer import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip, _hip.load_library(require_gpu=False)


def test_strip_entry_points_are_declared_exported_and_bound():
    _hip, lib = _library()
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(st_[a-z0-9_]+)\s*\(', text))
    for name in QN_SYMBOLS:
        assert 'lbfgs' not in name
        assert name in declared and hasattr(lib, name) and name in _hip.EXPORTED_SYMBOLS, name
    assert lib.st_abi_version() == 2                      # additions only
    for method in ('strip_dots', 'strip_apply', 'update_strip', 'step_strip'):
        assert callable(getattr(_hip.LBFGS, method))
    from style_transfer import sharding
    assert callable(sharding.lbfgs_lockstep) and 'ex.kind == 6' in inspect.getsource(sharding.DistFabric.apply)


def test_strip_state_is_the_unsharded_layout_plus_a_record_per_rank():
    _hip, lib = _library()
    for count in (1, 3 * 19 * 17, 3 * 64 * 64):
        sizes = [lib.st_qn_strip_state_bytes(count, w) for w in range(1, 9)]
        assert sizes[0] >= lib.st_lbfgs_state_bytes(count)
        steps = {b - a for a, b in zip(sizes, sizes[1:])}
        assert len(steps) == 1 and min(steps) > 0 and min(steps) % 16 == 0, steps
        assert min(steps) >= 72 * 8                       # 70 sums and one maximum in double, padded
        assert all(s % 16 == 0 for s in sizes)
    for count, world in ((0, 1), (-5, 2), (100, 0), (100, 9), (100, -1)):
        assert lib.st_qn_strip_state_bytes(count, world) == 0, (count, world)


def test_stylize_runs_sharded_lbfgs_through_the_library():
    from style_transfer import style_transfer
    src = inspect.getsource(style_transfer.StyleTransfer.stylize)
    code = '\n'.join(line.split('#')[0] for line in src.splitlines())
    assert 'StripLBFGS(' not in code and '.average.update(' not in code
    assert '_hip.LBFGS(self.image, rank, world)' in code and '.step_strip(' in code

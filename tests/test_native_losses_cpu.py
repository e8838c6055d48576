"""The native loss modules without a GPU: the C ABI carries the standalone head and the pointwise entries (header, library
and ctypes binding agree, still ABI version 2), and everything the native path does not take - CPU tensors, float64,
batches, other channel counts, a module whose buffers have another dtype - is refused by the eligibility function and runs
the torch code, bit for bit what it gives with the dispatch switched off."""
import os
import re

import pytest
import torch

from conftest import REPO

NEW_ENTRIES = ['st_head_create', 'st_head_destroy', 'st_head_device_bytes', 'st_head_state_floats', 'st_head_moments',
               'st_head_forward', 'st_head_backward', 'st_op_reduce_scratch_floats', 'st_op_mse_loss',
               'st_op_mse_loss_backward', 'st_op_scaled_mse_loss', 'st_op_scaled_mse_loss_backward', 'st_op_tv_value',
               'st_op_tv_loss_backward']


def test_header_library_and_binding_carry_the_new_entries():
    from style_transfer import _hip
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    assert re.search(r'#define\s+ST_AMD_ABI_VERSION\s+2\b', text)
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(st_[a-z0-9_]+)\s*\(', code))
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load_library(require_gpu=False)
    assert lib.st_abi_version() == 2
    for name in NEW_ENTRIES:
        assert name in declared, f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in _hip.EXPORTED_SYMBOLS, f'{name} is not declared by _hip._declare'
    assert callable(_hip.Head) and all(hasattr(_hip.Head, m) for m in ('moments', 'forward', 'backward', 'device_bytes', '__del__'))
    assert lib.st_op_reduce_scratch_floats() >= 4 * 2048


def _pair(shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype), (1.3 * torch.randn(shape, generator=g) + 0.2).to(dtype)


def _modules(x, t):
    from style_transfer import losses as L
    with L.native(False):           # (targets of CPU tensors are torch either way; be explicit)
        return {'w2': L.StyleLossW2(L.StyleLossW2.get_target(t)), 'gram': L.StyleLoss(L.StyleLoss.get_target(t)),
                'mse': L.ContentLossMSE(t), 'scaled_mse': L.ContentLoss(t)}


def _buffers(kind, module):
    return {'w2': lambda m: (m.mean, m.cov, m.cov_sqrt), 'gram': lambda m: (m.target,),
            'mse': lambda m: (m.target,), 'scaled_mse': lambda m: (m.target,)}[kind](module)


CASES = {
    'cpu tensor': ((1, 64, 5, 6), torch.float32),
    'float64': ((1, 64, 5, 6), torch.float64),
    'batch 2': ((2, 64, 5, 6), torch.float32),
    'C = 96': ((1, 96, 5, 6), torch.float32),
}


@pytest.mark.parametrize('case', list(CASES))
def test_ineligible_inputs_take_the_torch_code_unchanged(case):
    from style_transfer import losses as L
    shape, dtype = CASES[case]
    x, t = _pair(shape, dtype)
    for kind, module in _modules(x, t).items():
        assert not L.eligible(x, kind, _buffers(kind, module)), (case, kind)
        before = dict(L.native_calls)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with L.native(True):
            a = module(xa)
        with L.native(False):
            b = module(xb)
        assert torch.equal(a, b), (case, kind)
        a.backward()
        b.backward()
        assert torch.equal(xa.grad, xb.grad), (case, kind)
        assert L.native_calls == before and L.head_of(module) is None
    assert not L.eligible(x, 'moments') and not L.eligible(x[..., :3, :, :], 'tv')
    img = x[..., :3, :, :].contiguous()
    with L.native(True):
        a = L.TVLoss()(img)
    with L.native(False):
        b = L.TVLoss()(img)
    assert torch.equal(a, b)


def test_a_module_in_another_dtype_is_not_eligible():
    """A float64 module beside fp32 features, here on the CPU (where the input alone already decides; the same pair on the
    device, where the buffers' dtype decides, is in test_native_losses_gpu.py): refused, and the output is the torch code's."""
    from style_transfer import losses as L
    x, t = _pair((1, 64, 5, 6))
    for kind, module in _modules(x, t).items():
        module = module.double()
        assert all(b.dtype == torch.float64 for b in _buffers(kind, module))
        assert not L.eligible(x, kind, _buffers(kind, module)), kind
        if kind == 'w2':            # torch's own answer to float64 matrices times fp32 ones, on either side of the switch
            for on in (True, False):
                with L.native(on), pytest.raises(RuntimeError):
                    module(x)
            continue
        with L.native(True):
            a = module(x)
        with L.native(False):
            b = module(x)
        assert torch.equal(a, b) and a.dtype == torch.float64, kind


def test_the_switch_is_a_call_and_a_context_manager():
    from style_transfer import losses as L
    former = L.native.enabled
    try:
        L.native(False)
        assert L.native.enabled is False
        with L.native(True, precision='fp32'):
            assert L.native.enabled is True and L.native.precision == 'fp32'
        assert L.native.enabled is False and L.native.precision == 'fp16x3'
        with pytest.raises(ValueError):
            L.native(True, precision='bf16')
    finally:
        L.native(former)
    # module state is the reference's: the same buffers, nothing of the head in state_dict or repr
    x, t = _pair((1, 64, 5, 6))
    mods = _modules(x, t)
    assert sorted(mods['w2'].state_dict()) == ['cov', 'cov_sqrt', 'eps', 'mean']
    assert sorted(mods['gram'].state_dict()) == ['loss.eps', 'target']
    assert sorted(mods['scaled_mse'].state_dict()) == ['loss.eps', 'target']
    assert sorted(mods['mse'].state_dict()) == ['target']

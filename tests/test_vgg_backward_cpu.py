"""CPU checks of the differentiable trunk: st_plan_backward is declared, exported and bound with the documented argument
types, and the autograd node of VGGFeatures (VGGTrunkFunction) does its bookkeeping right - driven by a stub plan whose
forward / feature / backward are plain torch on a two-layer toy, so no GPU is needed."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import REPO


# ---- the C ABI and its binding ------------------------------------------------------------------------------------------
def test_backward_entry_is_declared_exported_and_bound():
    from style_transfer import _hip
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    assert ('int st_plan_backward(st_plan* plan, int count, const int* layers, const float* const* grads, '
            'float* grad_image, void* stream);') in flat
    assert '#define ST_AMD_ABI_VERSION 2' in header
    # the header comment names the reference lines it stands for and what the first call costs
    comment = header.split('int st_plan_backward(')[0].rsplit('/*', 1)[1]
    assert 'style_transfer.py:472-476' in comment and 'style_transfer.py:78-90' in comment and 'doubles' in comment
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.load_library(require_gpu=False)
    assert 'st_plan_backward' in _hip.EXPORTED_SYMBOLS
    fn = lib.st_plan_backward
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p]
    params = inspect.signature(_hip.Plan.backward).parameters
    assert list(params) == ['self', 'layers', 'grads', 'grad_out'] and params['grad_out'].default is None
    assert _hip.Plan.forward_count == 0


def test_entry_refuses_a_null_plan_without_a_gpu():
    """Argument checks come before any device work: callable here, and the failure has a text."""
    from style_transfer import _hip
    lib = _hip.load_library(require_gpu=False)
    assert lib.st_plan_backward(None, 1, None, None, None, None) != 0
    assert b'st_plan_backward' in lib.st_last_error()


# ---- the autograd node, on a stub plan ----------------------------------------------------------------------------------
class StubPlan:
    """conv3x3 -> ReLU (tap 1) -> conv3x3 -> ReLU (tap 3) in plain torch, with the duck type VGGTrunkFunction asks for:
    forward, feature, backward and forward_count.  Like a real plan it holds ONE forward's activations, and its backward
    differentiates whatever forward ran last."""

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.w1 = torch.randn((4, 3, 3, 3), generator=g) * 0.3
        self.w2 = torch.randn((5, 4, 3, 3), generator=g) * 0.3
        self.forward_count = 0
        self.backward_layers = []
        self.x = None

    def taps(self, x):
        t1 = torch.relu(torch.nn.functional.conv2d(x, self.w1, padding=1))
        return {1: t1, 3: torch.relu(torch.nn.functional.conv2d(t1, self.w2, padding=1))}

    def forward(self, x, last_layer=3):
        assert x.dtype == torch.float32 and not x.requires_grad
        self.forward_count += 1
        self.x = x.clone()
        with torch.no_grad():
            self.maps = self.taps(self.x)

    def feature(self, layer):
        return self.maps[layer].clone()

    def backward(self, layers, grads):
        assert all(g.dtype == torch.float32 and g.is_contiguous() for g in grads)
        self.backward_layers.append(list(layers))
        with torch.enable_grad():                 # (a once_differentiable backward runs with grad mode off)
            x = self.x.clone().requires_grad_(True)
            taps = self.taps(x)
        return torch.autograd.grad([taps[layer] for layer in layers], x, list(grads))[0]


def _stub_model(plan, height, width, layers=(1, 3)):
    """A VGGFeatures whose plan cache holds the stub (its constructor needs a GPU for the weights)."""
    from style_transfer.style_transfer import VGGFeatures
    model = object.__new__(VGGFeatures)
    model.layers, model.pooling, model.device, model.net = sorted(layers), 'max', torch.device('cpu'), None
    model._plans = {(height, width): plan}
    return model


def _image(seed, dtype=torch.float32):
    return torch.rand((1, 3, 6, 7), generator=torch.Generator().manual_seed(seed)).to(dtype)


def _reference(plan, image, loss_of):
    x = image.detach().clone().float().requires_grad_(True)
    loss_of({'input': x, **plan.taps(x)}).backward()
    return x.grad


def test_input_tap_is_the_callers_tensor_and_none_gradients_are_skipped():
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    image = _image(1).requires_grad_(True)
    feats = model(image)
    assert feats['input'] is image
    assert all('VGGTrunkFunction' in type(feats[k].grad_fn).__name__ for k in (1, 3))

    def loss_of(f):          # tap 1 is not used: its gradient arrives as None; 'input' flows through plain autograd
        return f[3].pow(2).sum() + f['input'].sum() * 0.5
    loss_of(feats).backward()
    assert plan.backward_layers == [[3]]
    assert torch.allclose(image.grad, _reference(plan, image, loss_of), rtol=1e-5, atol=1e-6)


def test_gradient_comes_back_in_the_inputs_dtype():
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    image = _image(2, torch.float64).requires_grad_(True)
    feats = model(image)

    def loss_of(f):
        return f[1].sum() + (f[3] * f[3]).sum()
    loss_of(feats).backward()
    assert image.grad.dtype == torch.float64 and image.grad.shape == image.shape
    assert plan.backward_layers == [[1, 3]]
    assert torch.allclose(image.grad.float(), _reference(plan, image, loss_of), rtol=1e-5, atol=1e-6)


def test_moved_forward_counter_triggers_exactly_one_recompute():
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    image = _image(3).requires_grad_(True)
    feats = model(image)

    def loss_of(f):
        return (f[1].pow(2).sum() + f[3].sum())
    loss = loss_of(feats)
    with torch.no_grad():
        model(_image(4))                          # e.g. the style image at the same size: the plan now holds ITS maps
    assert plan.forward_count == 2
    want = _reference(plan, image, loss_of)
    loss.backward(retain_graph=True)
    assert plan.forward_count == 3                # one recompute from the saved input ...
    assert torch.allclose(image.grad, want, rtol=1e-5, atol=1e-6)
    first, image.grad = image.grad.clone(), None
    loss.backward()                               # ... and none for the second pass over the same graph
    assert plan.forward_count == 3
    assert torch.equal(image.grad, first)


def test_retain_graph_twice_gives_the_same_gradient():
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    image = _image(5).requires_grad_(True)
    loss = model(image)[3].pow(2).sum()
    (a,) = torch.autograd.grad(loss, image, retain_graph=True)
    (b,) = torch.autograd.grad(loss, image, retain_graph=True)
    assert torch.equal(a, b) and plan.forward_count == 1 and plan.backward_layers == [[3], [3]]


def test_function_is_not_used_without_grad():
    """A regression guard, not evidence for the feature (it passes without it): with grad mode off, or an input that does
    not require grad, VGGFeatures behaves exactly as before - plain copies of the taps, no autograd node, no backward."""
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    image = _image(6)
    for feats in (model(image), ):                                  # the input does not require grad
        assert feats['input'] is image and all(feats[k].grad_fn is None and not feats[k].requires_grad for k in (1, 3))
    with torch.no_grad():                                           # it does, but grad mode is off
        feats = model(image.clone().requires_grad_(True))
    assert all(feats[k].grad_fn is None and not feats[k].requires_grad for k in (1, 3))
    assert plan.forward_count == 2 and plan.backward_layers == []


def test_double_backward_is_refused():
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    image = _image(7).requires_grad_(True)
    (g,) = torch.autograd.grad(model(image)[3].sum(), image, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_batches_are_refused():
    plan = StubPlan()
    model = _stub_model(plan, 6, 7)
    with pytest.raises(ValueError):
        model(torch.rand((2, 3, 6, 7)).requires_grad_(True))

"""The reference's loss / bookkeeping modules as importable ``nn.Module`` classes (API completeness, SURVEY.md
section 2 row 2).

``stylize()`` does not build a module graph: the closure of reference style_transfer.py:472-476 is one call into
libst_amd.so.  User code written against the reference can however import these names from
``style_transfer.style_transfer`` - ``ScaledMSELoss``, ``ContentLoss``, ``ContentLossMSE``, ``StyleLoss``,
``StyleLossW2``, ``TVLoss``, ``SumLoss``, ``Scale``, ``LayerApply``, ``eye_like`` (reference :93-234) - so they are
provided here with the reference's constructor arguments, buffers, static helpers and arithmetic.  ``LaplacianLoss`` is this
project's own (include/st_amd.h fixes its semantics): the module form of ``st_plan_set_laplacian``'s term, dispatched like the
others - one dense fp32 HIP image, any channel count, runs st_op_laplacian_value / st_op_laplacian_backward per pool size.
``StyleLossW2Diag`` is this project's own too: ``StyleLossW2`` with both covariances restricted to their diagonals, the module
form of ``st_plan_set_w2_diagonal``'s term - one dense fp32 HIP tensor, any channel count, runs st_op_w2_diag_loss /
st_op_w2_diag_loss_backward.
``StyleLossW2Marginal`` is the module form of ``st_plan_set_w2_marginal``'s term: per channel the sorted tap against the style's
sorted tap - one dense fp32 HIP tensor, any channel count, runs st_op_w2_marginal_loss / st_op_w2_marginal_loss_backward.
``StyleLossNearest`` is the module form of ``st_plan_set_style_nearest``'s term: every feature vector of the input against the
closest of the style's feature vectors - one dense fp32 HIP tensor whose channel count is a multiple of 32 runs st_op_nearest_loss /
st_op_nearest_loss_backward.
``StyleLossSliced`` is the module form of ``st_plan_set_style_sliced``'s term: the sorted projections of the input onto random unit
directions against the style's, new directions at every forward in training mode - one dense fp32 HIP tensor whose channel count is
a multiple of 64 runs st_op_sliced_directions / st_op_sliced_target / st_op_sliced_loss / st_op_sliced_loss_backward.

Native dispatch.  On an ELIGIBLE tensor (``eligible`` below: one dense fp32 tensor on a HIP device, batch 1 or absent, 64 /
128 / 256 / 512 channels for the style modules, the module's buffers beside it in fp32) the five loss modules run in the
library instead of torch kernels: a standalone style head (``_hip.Head``: st_head_* in include/st_amd.h) behind
``StyleLossW2`` / ``StyleLoss``, the pointwise entries (st_op_mse_loss, st_op_scaled_mse_loss, st_op_tv_value and their
``_backward`` twins) behind ``ContentLossMSE`` / ``ContentLoss`` / ``ScaledMSELoss`` / ``TVLoss`` - one
``torch.autograd.Function`` per kind, whose backward hands autograd's ``grad_output`` to the library as a device scalar.
Everything else - CPU tensors, float64, batches, other channel counts, a backward under ``create_graph=True`` - is the
plain torch code below, unchanged.  What a call keeps for its backward lives on its autograd node (the input, and the
C x C-sized (Ssym, b) of a style head or the two totals of a scaled MSE), so a module may be applied any number of times
before ``backward()``; a module's head - workspaces only - is created on first use per (C, h, w), replaced when the shape
changes, and is no part of ``state_dict()``.  ``native(enabled)`` switches the dispatch, also as a context manager.
One host synchronisation per module, not per call: the kernels take ``eps`` as an argument, so a module's ``eps`` buffer is read
back on its first native call (``_eps_of``).
"""

import weakref
from functools import partial

import torch
from torch import nn
from torch.nn import functional as F

from . import sqrtm

HEAD_CHANNELS = (64, 128, 256, 512)


class native:
    """``losses.native(False)`` sends every module down the torch path, ``losses.native(True)`` back to the library;
    ``with losses.native(False): ...`` restores the former setting afterwards.  ``precision``: the arithmetic of the style
    heads' matrix kernels, 'fp16x3' (the shipped default of the trunk) or 'fp32'."""

    enabled = True
    precision = 'fp16x3'

    def __init__(self, enabled=True, precision=None):
        if precision not in (None, 'fp16x3', 'fp32'):
            raise ValueError(f"precision {precision!r}: must be 'fp16x3' or 'fp32'")
        self._former = (native.enabled, native.precision)
        native.enabled = bool(enabled)
        if precision is not None:
            native.precision = precision

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        native.enabled, native.precision = self._former


# calls that went to the library, by kind ('w2', 'gram', 'mse', 'scaled_mse', 'tv', 'laplacian', 'w2_diag', 'w2_marginal', 'nearest', 'nearest_cosine', 'sliced', 'moments'): the native indicator of the
# modules that hold no head
native_calls = {}
_prepared_sets = weakref.WeakKeyDictionary()       # StyleLossNearest module -> (target, version, its prepared style set), kept off the module as the heads are
_heads = weakref.WeakKeyDictionary()       # module -> its _hip.Head (no module attribute: deepcopy / pickle / state_dict never see it)
_target_heads = {}                         # get_target's moments-only heads (the static helpers have no module), the six most
                                           # recent shapes; release_target_heads() frees them


def _count(kind):
    native_calls[kind] = native_calls.get(kind, 0) + 1


def _one_dense_fp32(t, trailing):
    """A strided fp32 tensor on a HIP device whose dimensions in front of the last ``trailing`` are absent or all 1."""
    return (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided
            and t.ndim >= trailing and t.numel() > 0 and all(d == 1 for d in t.shape[:t.ndim - trailing]))


def _buffer_ok(b, like, numel):
    return (torch.is_tensor(b) and b.device == like.device and b.dtype == torch.float32 and b.numel() == numel
            and b.is_contiguous() and b.data_ptr() % 16 == 0 and not b.requires_grad)


def _max_pixels():
    """The library's one size limit (include/st_amd.h, "Size limit"; st_max_pixels): the pixels a map may hold."""
    from . import _hip
    return _hip.max_pixels()


def _pixels_ok(input):
    return input.shape[-2] * input.shape[-1] <= _max_pixels()


def eligible(input, kind, buffers=()):
    """Can ``input`` take the native path of ``kind`` ('w2', 'gram', 'mse', 'scaled_mse', 'tv', 'laplacian', 'moments')?  ``buffers``: the
    module's tensors that the library would read in place - (mean, cov, cov_sqrt), (gram target,) or (target,).  Says nothing
    about the ``native`` switch."""
    if kind in ('w2', 'gram', 'moments'):
        if not (_one_dense_fp32(input, 3) and input.ndim in (3, 4) and input.shape[-3] in HEAD_CHANNELS):
            return False
        if not _pixels_ok(input):
            return False
        c = input.shape[-3]
        sizes = {'w2': (c, c * c, c * c), 'gram': (c * c,), 'moments': ()}[kind]
    elif kind == 'w2_diag':
        # (any channel count the launch's grid takes; buffers: none, or the module's (mean, std))
        if not (_one_dense_fp32(input, 3) and input.ndim in (3, 4) and input.shape[-3] <= 65535 and _pixels_ok(input)):
            return False
        sizes = (input.shape[-3],) * len(buffers)
    elif kind == 'w2_marginal':
        # (any channel count; buffers: none, or the module's target resampled to the input's pixel count)
        if not (_one_dense_fp32(input, 3) and input.ndim in (3, 4) and input.shape[-2] * input.shape[-1] < 1 << 32):
            return False
        sizes = (input.shape[-3] * input.shape[-2] * input.shape[-1],) * len(buffers)
    elif kind == 'nearest':
        # (a channel count that is a multiple of the search kernel's K chunk; buffers: none)
        if not (_one_dense_fp32(input, 3) and input.ndim in (3, 4) and input.shape[-3] >= 32 and input.shape[-3] % 32 == 0 and
                input.shape[-2] * input.shape[-1] < 1 << 31):
            return False
        sizes = ()
    elif kind == 'sliced':
        # (a channel count that is a multiple of 64; buffers: none)
        if not (_one_dense_fp32(input, 3) and input.ndim in (3, 4) and input.shape[-3] % 64 == 0 and
                _pixels_ok(input)):
            return False
        sizes = ()
    elif kind == 'tv':
        if not (_one_dense_fp32(input, 3) and input.ndim in (3, 4) and input.shape[-3] == 3 and _pixels_ok(input)):
            return False
        sizes = ()
    elif kind == 'laplacian':
        # (buffers: one target per pool size, each of its own size - checked by the module, which knows the pools)
        return _one_dense_fp32(input, 3) and input.ndim in (3, 4) and _pixels_ok(input) and input.numel() < 1 << 31 and \
            all(_buffer_ok(b, input, b.numel()) for b in buffers)
    else:
        if not (torch.is_tensor(input) and _one_dense_fp32(input, min(input.ndim, 3))):
            return False
        sizes = (input.numel(),)
        if len(buffers) != 1 or not torch.is_tensor(buffers[0]) or buffers[0].shape != input.shape:
            return False
    return len(buffers) == len(sizes) and all(_buffer_ok(b, input, n) for b, n in zip(buffers, sizes))


def _wants_grad(t):
    """Will autograd ask this call for a gradient?  (Under torch.no_grad() it will not, whatever t.requires_grad says.)"""
    return torch.is_grad_enabled() and t.requires_grad


def _dense(t):
    """The tensor as the library reads it: contiguous, on a 16-byte boundary."""
    t = t.detach().contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _torch_vjp(torch_forward, input, grad_output):
    """A backward that is itself being differentiated (``create_graph=True``): the torch code's gradient, as a graph."""
    with torch.enable_grad(), native(False):
        (grad,) = torch.autograd.grad(torch_forward(input), input, grad_output, create_graph=True)
    return grad


def _eps_of(module):
    """The module's ``eps`` buffer as a float (the kernels take it as an argument).  Reading it is a device-to-host copy,
    i.e. a synchronisation: done on the module's first native call and again only when the buffer is another tensor object
    (``.to()``, ``register_buffer``) or has been written in place (``load_state_dict``; the version counter).  The cache
    holds the tensor itself, so no other buffer can turn up at its address.  (``module.eps.data = ...`` goes unnoticed.)"""
    eps = module.eps
    cached = module.__dict__.get('_eps_cache')
    if cached is None or cached[0] is not eps or cached[1] != eps._version:
        cached = module.__dict__['_eps_cache'] = (eps, eps._version, float(eps))
    return cached[2]


def _new_head(kind, x):
    from . import _hip
    return _hip.Head(kind, x.shape[-3], x.shape[-2], x.shape[-1], x.device, native.precision)


def _head_matches(head, kind, x):
    return (head is not None and head.kind == kind and head.shape == tuple(x.shape[-3:]) and head.device == x.device
            and head.precision == native.precision)


def _module_head(module, kind, x):
    head = _heads.get(module)
    if not _head_matches(head, kind, x):
        head = _heads[module] = _new_head(kind, x)
    return head


def head_of(module):
    """The style head a ``StyleLossW2`` / ``StyleLoss`` currently holds (``_hip.Head``), or None: it has not run natively."""
    return _heads.get(module)


def release_target_heads():
    """Free the moments-only heads that ``get_target`` keeps for its six most recent shapes (a Gram workspace each, at most
    64 MiB); the next call creates what it needs again."""
    _target_heads.clear()


def _native_moments(target, want_mean):
    """(mean or None, srm) of an eligible tensor through a head's moments entry, in the shapes the torch code returns."""
    x = _dense(target)
    key = (tuple(x.shape[-3:]), x.device, native.precision)
    head = _target_heads.pop(key, None) or _new_head('moments', x)
    _target_heads[key] = head                      # most recent last
    while len(_target_heads) > 6:
        _target_heads.pop(next(iter(_target_heads)))
    _count('moments')
    mean, srm = head.moments(x, mean=want_mean)
    c = x.shape[-3]
    lead = tuple(target.shape[:-3])
    return (mean.view(*lead, c) if want_mean else None), srm.view(*lead, c, c)


class _HeadLoss(torch.autograd.Function):
    """A style head's unweighted loss.  Saved on the node: the input (autograd's version check stays in force) and the
    head's per-call state, (Ssym, b) + the operand bound; the tap-sized gradient is made in backward() only."""

    @staticmethod
    def forward(ctx, input, module, kind, targets, eps, need_grad):
        # need_grad: decided by the module (_wants_grad) - grad mode is always off in here, and ctx.needs_input_grad says
        # input.requires_grad whatever the caller's grad mode is
        x = _dense(input)
        head = _module_head(module, kind, x)
        loss, state = head.forward(x, targets, eps, need_grad=need_grad)
        _count(kind)
        if need_grad:
            ctx.save_for_backward(input, state)
            ctx.head = head                        # (the module may move on to another shape before this node's backward)
            ctx.torch_forward = module._forward_torch
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        input, state = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None, None, None, None
        grad = ctx.head.backward(_dense(input), state, grad_output.contiguous())
        return grad.view(input.shape), None, None, None, None, None


class _W2HeadLoss(_HeadLoss):
    """StyleLossW2.forward (reference :174-181) on the library's head."""


class _GramHeadLoss(_HeadLoss):
    """StyleLoss.forward (reference :141-142) on the library's head."""


class _MSELoss(torch.autograd.Function):
    """nn.MSELoss (reference :119-126): st_op_mse_loss / st_op_mse_loss_backward."""

    @staticmethod
    def forward(ctx, input, target):
        from . import _hip
        loss = _hip.op_mse_loss(_dense(input), target)
        _count('mse')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, target)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, target = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(lambda x: F.mse_loss(x, target), input, grad_output), None
        return _hip.op_mse_loss_backward(_dense(input), target, grad_output.contiguous()).view(input.shape), None


class _ScaledMSELoss(torch.autograd.Function):
    """ScaledMSELoss.forward (reference :104-106): st_op_scaled_mse_loss; the two totals stay on the node for
    st_op_scaled_mse_loss_backward."""

    @staticmethod
    def forward(ctx, input, target, module, eps):
        from . import _hip
        loss, totals = _hip.op_scaled_mse_loss(_dense(input), target, eps)
        _count('scaled_mse')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, target, totals)
            ctx.torch_forward = lambda x: module._forward_torch(x, target)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, target, totals = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None, None
        grad = _hip.op_scaled_mse_loss_backward(_dense(input), target, totals, grad_output.contiguous())
        return grad.view(input.shape), None, None, None


class _W2DiagLoss(torch.autograd.Function):
    """StyleLossW2Diag.forward: st_op_w2_diag_loss; the 2 C coefficients of the gradient stay on the node for
    st_op_w2_diag_loss_backward."""

    @staticmethod
    def forward(ctx, input, module, mean, std, eps):
        from . import _hip
        loss, coeffs = _hip.op_w2_diag_loss(_dense(input), mean, std, eps)
        _count('w2_diag')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, coeffs)
            ctx.torch_forward = module._forward_torch
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, coeffs = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None, None, None
        grad = _hip.op_w2_diag_loss_backward(_dense(input), coeffs, grad_output.contiguous())
        return grad.view(input.shape), None, None, None, None


class _W2MarginalLoss(torch.autograd.Function):
    """StyleLossW2Marginal.forward: st_op_w2_marginal_loss; the gradient at weight 1 - written through the sort's permutation
    by the same pass - stays on the node for st_op_w2_marginal_loss_backward."""

    @staticmethod
    def forward(ctx, input, module, target):
        from . import _hip
        loss, unit = _hip.op_w2_marginal_loss(_dense(input), target)
        _count('w2_marginal')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, unit)
            ctx.torch_forward = module._forward_torch
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, unit = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None
        grad = _hip.op_w2_marginal_loss_backward(unit, grad_output.contiguous())
        return grad.view(input.shape), None, None


class _NearestLoss(torch.autograd.Function):
    """StyleLossNearest.forward: st_op_nearest_loss; the gradient at weight 1 - written by the finish pass with the matches held
    constant - stays on the node for st_op_nearest_loss_backward."""

    @staticmethod
    def forward(ctx, input, module, prepared, m):
        from . import _hip
        loss, unit, _ = _hip.op_nearest_loss(_dense(input), prepared, m)
        _count('nearest')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, unit)
            ctx.torch_forward = module._forward_torch
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, unit = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None, None
        grad = _hip.op_nearest_loss_backward(unit, grad_output.contiguous())
        return grad.view(input.shape), None, None, None


class _NearestCosineLoss(_NearestLoss):
    """StyleLossNearest.forward under the 'cosine' and 'centered_cosine' metrics: st_op_nearest_cosine_loss; the backward is
    _NearestLoss's."""

    @staticmethod
    def forward(ctx, input, module, prepared, m):
        from . import _hip
        loss, unit, _ = _hip.op_nearest_cosine_loss(_dense(input), prepared, m)
        _count('nearest_cosine')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, unit)
            ctx.torch_forward = module._forward_torch
        return loss


class _SlicedLoss(torch.autograd.Function):
    """StyleLossSliced.forward: st_op_sliced_loss under the given directions; the gradient at weight 1 - the back-projection of
    the residual, directions and permutations held constant - stays on the node for st_op_sliced_loss_backward."""

    @staticmethod
    def forward(ctx, input, module, r, rt, target):
        from . import _hip
        loss, unit = _hip.op_sliced_loss(_dense(input), r, rt, target)
        _count('sliced')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, unit)
            ctx.torch_forward = lambda x: module._forward_torch(x, r)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, unit = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None, None, None
        grad = _hip.op_sliced_loss_backward(unit, grad_output.contiguous())
        return grad.view(input.shape), None, None, None, None


class _TVLoss(torch.autograd.Function):
    """TVLoss.forward (reference :187-195): st_op_tv_value / st_op_tv_loss_backward."""

    @staticmethod
    def forward(ctx, input, module):
        from . import _hip
        loss = _hip.op_tv_value(_dense(input))
        _count('tv')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input)
            ctx.torch_forward = module._forward_torch
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None
        return _hip.op_tv_loss_backward(_dense(input), grad_output.contiguous()).view(input.shape), None


class _LaplacianLoss(torch.autograd.Function):
    """LaplacianLoss.forward: st_op_laplacian_value per pool size, the values added in list order; the residuals are what
    st_op_laplacian_backward needs."""

    @staticmethod
    def forward(ctx, input, module, targets):
        from . import _hip
        x = _dense(input)
        loss, residuals = None, []
        for pool, target in zip(module.pools, targets):
            value, residual = _hip.op_laplacian_value(x, target, pool)
            loss = value if loss is None else loss + value
            residuals.append(residual)
        _count('laplacian')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, *residuals)
            ctx.torch_forward = module._forward_torch
            ctx.pools = module.pools
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _hip
        input, *residuals = ctx.saved_tensors
        if torch.is_grad_enabled():
            return _torch_vjp(ctx.torch_forward, input, grad_output), None, None
        upstream = grad_output.contiguous()
        grad = None
        for pool, residual in zip(ctx.pools, residuals):
            part = _hip.op_laplacian_backward(residual, input.shape, pool, upstream)
            grad = part if grad is None else grad + part
        return grad, None, None


class ScaledMSELoss(nn.Module):
    """Sum of squared differences over the L1 norm of the difference (+ eps): an MSE whose gradient has an L1
    norm of about one (reference :93-106)."""

    def __init__(self, eps=1e-8):
        super().__init__()
        self.register_buffer('eps', torch.tensor(eps))

    def extra_repr(self):
        return f'eps={self.eps:g}'

    def _forward_torch(self, input, target):
        delta = input - target
        return delta.pow(2).sum() / delta.abs().sum().add(self.eps)

    def forward(self, input, target):
        if native.enabled and eligible(input, 'scaled_mse', (target,)) and _buffer_ok(self.eps, input, 1):
            return _ScaledMSELoss.apply(input, target, self, _eps_of(self))
        return self._forward_torch(input, target)


class _TargetLoss(nn.Module):
    """loss(transform(input), target) with the target held as a buffer."""

    def __init__(self, target, loss):
        super().__init__()
        self.register_buffer('target', target)
        self.loss = loss

    def forward(self, input):
        return self.loss(input, self.target)


class ContentLoss(_TargetLoss):
    """Reference :109-116."""

    def __init__(self, target, eps=1e-8):
        super().__init__(target, ScaledMSELoss(eps=eps))


class ContentLossMSE(_TargetLoss):
    """Reference :119-126 - the content term stylize() uses (in the library: content_mse_kernel)."""

    def __init__(self, target):
        super().__init__(target, nn.MSELoss())

    def forward(self, input):
        if native.enabled and eligible(input, 'mse', (self.target,)):
            return _MSELoss.apply(input, self.target)
        return self.loss(input, self.target)


class StyleLoss(_TargetLoss):
    """Gram-matrix style loss (reference :129-142); the Gram matrix is divided by the number of positions."""

    def __init__(self, target, eps=1e-8):
        super().__init__(target, ScaledMSELoss(eps=eps))

    @staticmethod
    def get_target(target):
        if native.enabled and eligible(target, 'moments') and not _wants_grad(target):
            return _native_moments(target, False)[1]
        return StyleLoss._get_target_torch(target)

    @staticmethod
    def _get_target_torch(target):
        flat = target.flatten(-2)
        return flat @ flat.transpose(-2, -1) / flat.shape[-1]

    def _forward_torch(self, input):
        return self.loss._forward_torch(self._get_target_torch(input), self.target)

    def forward(self, input):
        if native.enabled and eligible(input, 'gram', (self.target,)) and _buffer_ok(self.loss.eps, input, 1):
            return _GramHeadLoss.apply(input, self, 'gram', (self.target,), _eps_of(self.loss), _wants_grad(input))
        return self._forward_torch(input)


def eye_like(x):
    return torch.eye(x.shape[-2], x.shape[-1], dtype=x.dtype, device=x.device).expand_as(x)


class StyleLossW2(nn.Module):
    """Wasserstein-2 distance between the Gaussians fitted to the input's and the target's features
    (reference :149-181; in the library: st_gram.hip + the Newton-Schulz chains)."""

    def __init__(self, target, eps=1e-4):
        super().__init__()
        self.sqrtm = partial(sqrtm.sqrtm_ns_lyap, num_iters=12)
        mean, srm = target
        cov = self.srm_to_cov(mean, srm) + eye_like(srm) * eps
        self.register_buffer('mean', mean)
        self.register_buffer('cov', cov)
        self.register_buffer('cov_sqrt', self.sqrtm(cov))
        self.register_buffer('eps', mean.new_tensor(eps))

    @staticmethod
    def get_target(target):
        """(mean, second raw moment) over the spatial positions - linear in the features' distribution, so targets
        of several style images can be blended."""
        if native.enabled and eligible(target, 'moments') and not _wants_grad(target):
            return _native_moments(target, True)
        return StyleLossW2._get_target_torch(target)

    @staticmethod
    def _get_target_torch(target):
        positions = target.shape[-2] * target.shape[-1]
        mean = target.mean([-2, -1])
        srm = torch.einsum('...chw,...dhw->...cd', target, target) / positions
        return mean, srm

    @staticmethod
    def srm_to_cov(mean, srm):
        return srm - torch.einsum('...c,...d->...cd', mean, mean)

    def forward(self, input):
        if native.enabled and eligible(input, 'w2', (self.mean, self.cov, self.cov_sqrt)) and _buffer_ok(self.eps, input, 1):
            return _W2HeadLoss.apply(input, self, 'w2', (self.mean, self.cov, self.cov_sqrt), _eps_of(self), _wants_grad(input))
        return self._forward_torch(input)

    def _forward_torch(self, input):
        mean, srm = self._get_target_torch(input)
        cov = self.srm_to_cov(mean, srm) + eye_like(srm) * self.eps
        mean_term = torch.mean((mean - self.mean) ** 2)
        cross = self.sqrtm(self.cov_sqrt @ cov @ self.cov_sqrt)
        cov_term = torch.diagonal(self.cov + cov - 2 * cross, dim1=-2, dim2=-1).mean()
        return mean_term + cov_term


class StyleLossW2Diag(nn.Module):
    """``StyleLossW2`` with both covariances restricted to their diagonals: for two Gaussians with diagonal covariances W2^2 is
    ``sum_c (mu - mu_t)^2 + sum_c (sigma - sigma_t)^2`` - the mean / standard-deviation (batch-norm statistics) loss of Li et
    al., "Demystifying Neural Style Transfer", the statistic AdaIN matches - here divided by the channel count as ``StyleLossW2``
    takes means.  Not in the reference; include/st_amd.h (st_plan_set_w2_diagonal) fixes the semantics:
    ``sigma = sqrt(max(q - mu^2, 0) + eps)`` with ``q`` the channel's second raw moment, the variance term as
    ``(sigma - sigma_t)^2`` so that the target's own features give exactly 0 with an exactly zero gradient, and a zero gradient
    through ``sigma`` where it is 0.  ``target`` = (mean [..., C], srm) with ``srm`` of shape [..., C] or [..., C, C] (its
    diagonal is taken), so a ``StyleLossW2`` target serves.  The torch path serves any device, dtype and batch; one dense fp32
    HIP tensor of any channel count runs in the library (st_w2diag.hip: two memory-bound launches, no C x C work)."""

    def __init__(self, target, eps=1e-4):
        super().__init__()
        mean, srm = target
        if srm.ndim == mean.ndim + 1:
            srm = torch.diagonal(srm, dim1=-2, dim2=-1)
        if srm.shape != mean.shape:
            raise ValueError(f'target of shapes {tuple(mean.shape)} and {tuple(srm.shape)}: (mean [..., C], srm [..., C] or [..., C, C])')
        eps = mean.new_tensor(eps)
        self.register_buffer('mean', mean)
        self.register_buffer('std', self._std(mean, srm, eps))
        self.register_buffer('eps', eps)

    @staticmethod
    def get_target(target):
        """(mean, the diagonal of the second raw moment) over the spatial positions - like ``StyleLossW2``'s target linear
        in the features' distribution, so targets of several style images can be blended."""
        if native.enabled and eligible(target, 'w2_diag') and not _wants_grad(target):
            from . import _hip
            _count('moments')
            mean, srm = _hip.op_channel_moments(_dense(target))
            shape = tuple(target.shape[:-2])
            return mean.view(shape), srm.view(shape)
        return StyleLossW2Diag._get_target_torch(target)

    @staticmethod
    def _get_target_torch(target):
        return target.mean([-2, -1]), (target * target).mean([-2, -1])

    @staticmethod
    def _std(mean, srm, eps):
        var = srm - mean * mean
        var = var + (var.clamp(min=0) - var).detach()       # max(var, 0) in value; the gradient passes as the header states it
        v = var + eps
        positive = v > 0
        return torch.where(positive, v, torch.ones_like(v)).sqrt() * positive.to(v.dtype)

    def forward(self, input):
        if native.enabled and eligible(input, 'w2_diag', (self.mean, self.std)) and _buffer_ok(self.eps, input, 1):
            return _W2DiagLoss.apply(input, self, self.mean, self.std, _eps_of(self))
        return self._forward_torch(input)

    def _forward_torch(self, input):
        mean, srm = self._get_target_torch(input)
        std = self._std(mean, srm, self.eps)
        return torch.mean((mean - self.mean) ** 2) + torch.mean((std - self.std) ** 2)


class StyleLossW2Marginal(nn.Module):
    """The W2 distance between the exact one-dimensional marginals of the input's channels and of a style tap's: per channel
    the sorted input against the style's sorted tap, ``mean((sort(f) - T)^2)`` - Risser et al.'s histogram loss in its exact
    form, the sliced Wasserstein loss of Heitz et al. along the channel axes (a user's own projections compose as
    ``R @ F`` in front).  Not in the reference; include/st_amd.h (st_plan_set_w2_marginal) fixes the semantics: the sort is
    the stable ascending one of ``f + 0.0``, its permutation a constant of the gradient, and ``T`` is the target's quantile
    function at the input's pixel count (``resample``: midpoint convention, a copy when the counts agree), so the target's own
    features give exactly 0 with an exactly zero gradient.  ``target`` = [C, n_q], sorted rows (``get_target``).  The torch
    path serves any device, dtype and batch; one dense fp32 HIP tensor of any channel count runs in the library
    (st_sort.hip: a segmented sort and one residual pass)."""

    def __init__(self, target):
        super().__init__()
        if target.ndim != 2:
            raise ValueError(f'target of shape {tuple(target.shape)}: [C, n_q], every row sorted')
        self.register_buffer('target', target)

    @staticmethod
    def get_target(target):
        """The sorted rows of the features, [..., C, h w]: every channel's quantile function.  Quantile functions resampled to
        one length (``resample``) can be blended, as moments can."""
        if native.enabled and eligible(target, 'w2_marginal') and not _wants_grad(target):
            from . import _hip
            _count('moments')
            values, _ = _hip.op_channel_sort(_dense(target), indices=False)
            return values.view(*target.shape[:-2], -1)
        return StyleLossW2Marginal._get_target_torch(target)

    @staticmethod
    def _get_target_torch(target):
        return torch.sort(target.flatten(-2) + 0.0, dim=-1, stable=True).values

    @staticmethod
    def resample(q, n):
        """Quantile functions q [..., n_q] at n midpoints: ``lerp(q, u)`` with ``u = clamp((i + 1/2) n_q / n - 1/2, 0, n_q - 1)``
        evaluated in float64, linear between ``floor(u)`` and ``floor(u) + 1`` in q's dtype."""
        n_q = q.shape[-1]
        if n_q == n:
            return q
        u = ((torch.arange(n, dtype=torch.float64, device=q.device) + 0.5) * n_q / n - 0.5).clamp(0, n_q - 1)
        i0 = u.floor().long()
        i1 = (i0 + 1).clamp(max=n_q - 1)
        t = (u - i0).to(q.dtype)
        a, b = q[..., i0], q[..., i1]
        return torch.where(t == 0, a, a + t * (b - a))

    def _target_for(self, input):
        """The target at the input's pixel count, resampled once per (count, target buffer, version)."""
        n = input.shape[-2] * input.shape[-1]
        target = self.target
        if target.shape[-1] == n:
            return target
        cached = self.__dict__.get('_resampled')
        if cached is None or cached[0] is not target or cached[1] != target._version or cached[2].shape[-1] != n:
            if native.enabled and _one_dense_fp32(target, 2) and target.is_contiguous():
                from . import _hip
                resampled = _hip.op_resample_quantiles(target, n)
            else:
                resampled = self.resample(target, n)
            cached = self.__dict__['_resampled'] = (target, target._version, resampled)
        return cached[2]

    def forward(self, input):
        if native.enabled and eligible(input, 'w2_marginal') and self.target.shape[0] == input.shape[-3] and \
                not self.target.requires_grad and self.target.device == input.device and self.target.dtype == torch.float32:
            target = self._target_for(input)
            if eligible(input, 'w2_marginal', (target,)):
                return _W2MarginalLoss.apply(input, self, target)
        return self._forward_torch(input)

    def _forward_torch(self, input):
        n = input.shape[-2] * input.shape[-1]
        values = torch.sort(input.flatten(-2) + 0.0, dim=-1, stable=True).values
        return torch.mean((values - self.resample(self.target, n)) ** 2)


class StyleLossNearest(nn.Module):
    """Nearest-neighbour feature matching: every feature vector ``f_i`` of the input against the closest of a style tap's
    feature vectors, ``mean_i,c (f_i - s_k*(i))^2`` with ``k*(i) = argmin_k |f_i - s_k|^2`` (ties: the lowest k) - the MRF /
    neural-neighbour family of style losses (Li & Wand's CNNMRF, Kolkin et al.'s NNST) in its L2 form, the one-sided Chamfer
    distance from the input to the style set.  Not in the reference; include/st_amd.h (st_plan_set_style_nearest) fixes the
    semantics: the match is a constant of the gradient (the a.e. derivative of the minimum), there is no eps, and nothing is
    resampled - ``target`` = [C, M] with any M (``get_target``).  The cost is ``2 C N M`` flop per call.  The torch path serves
    any device, dtype and batch, chunked over the pixels so that no N x M matrix exists; one dense fp32 HIP tensor whose channel
    count is a multiple of 32 runs in the library (st_nearest.hip: one fused search, which writes no score, and one finish
    pass; the search runs in fp16x3, so a match is optimal up to that arithmetic).
    ``metric``: 'l2' (the above), 'cosine' or 'centered_cosine' - the metrics the family is named after
    (st_plan_set_nearest_metric): with ``mu`` = 0 or the mean of the target's columns, ``s^_k = (s_k - mu) / sqrt(|s_k - mu|^2 +
    1e-8)``, ``g_i = f_i - mu`` and ``k*(i) = argmax_k <g_i, s^_k>`` (the first maximum), the term is ``mean_i (1 - <g_i, s^_k*> /
    sqrt(|g_i|^2 + 1e-8))``: one minus the cosine to the best-matching style vector, which is what that search minimises.  The
    match and ``mu`` are constants of the gradient.  On the device these calls count under 'nearest_cosine'."""

    chunk = 4096        # pixels per block of the torch path's distance matrix
    eps = 1e-8          # of the cosine metrics; not an argument (include/st_amd.h)

    def __init__(self, target, metric='l2'):
        super().__init__()
        if target.ndim != 2:
            raise ValueError(f'target of shape {tuple(target.shape)}: [C, M], the style feature vectors as columns')
        from . import _hip
        if metric not in _hip.NEAREST_METRICS:
            raise ValueError(f'metric {metric!r}: one of {_hip.NEAREST_METRICS}')
        self.metric = metric
        self.register_buffer('target', target)

    @staticmethod
    def get_target(target):
        """The flattened features, [..., C, h w]: every pixel's feature vector as a column.  Several style images give the
        union of their vectors: concatenate along the last axis."""
        return target.flatten(-2)

    @staticmethod
    def match(feat, target, chunk=4096):
        """k*(i) for feat [..., C, N] against target [C, M], [..., N] int64: the arg-min of ``|f_i - s_k|^2`` evaluated as
        ``|s_k|^2 / 2 - <f_i, s_k>``, the first minimum."""
        half = 0.5 * (target * target).sum(0)
        out = []
        for start in range(0, feat.shape[-1], chunk):
            f = feat[..., start:start + chunk]
            out.append(_first_argmin(half[:, None] - torch.einsum('ck,...cn->...kn', target, f), dim=-2))
        return torch.cat(out, dim=-1)

    def _prepared(self):
        """The target as the kernels read it, made once per (target buffer, version); kept beside the module, not on it, so
        deepcopy / pickle / state_dict never see it."""
        target = self.target
        cached = _prepared_sets.get(self)
        if cached is None or cached[0] is not target or cached[1] != target._version:
            from . import _hip
            if self.metric == 'l2':
                prepared = _hip.op_nearest_prepare(target.contiguous())
            else:
                prepared = _hip.op_nearest_cosine_prepare(target.contiguous(), centered=self.metric == 'centered_cosine')
            cached = _prepared_sets[self] = (target, target._version, prepared)
        return cached[2]

    def forward(self, input):
        if native.enabled and eligible(input, 'nearest') and self.target.shape[0] == input.shape[-3] and \
                not self.target.requires_grad and self.target.device == input.device and self.target.dtype == torch.float32:
            if self.metric == 'l2':
                return _NearestLoss.apply(input, self, self._prepared(), int(self.target.shape[1]))
            if _pixels_ok(input) and self.target.shape[1] <= _max_pixels():
                return _NearestCosineLoss.apply(input, self, self._prepared(), int(self.target.shape[1]))
        return self._forward_torch(input)

    def cosine_parts(self, dtype):
        """(mu [C], the unit vectors s^ [C, M]) of the cosine metrics, from ``target`` in ``dtype``."""
        s = self.target.to(dtype)
        mu = s.mean(1) if self.metric == 'centered_cosine' else torch.zeros_like(s[:, 0])
        d = s - mu[:, None]
        return mu, d / torch.sqrt((d * d).sum(0) + self.eps)

    @staticmethod
    def match_cosine(g, unit, chunk=4096):
        """k*(i) for the centred features g [..., C, N] against the unit vectors [C, M], [..., N] int64: the first maximum of
        ``<g_i, s^_k>``."""
        out = []
        for start in range(0, g.shape[-1], chunk):
            out.append(_first_argmin(-torch.einsum('ck,...cn->...kn', unit, g[..., start:start + chunk]), dim=-2))
        return torch.cat(out, dim=-1)

    def _forward_torch(self, input):
        feat = input.flatten(-2)
        if self.metric != 'l2':
            mu, unit = self.cosine_parts(feat.dtype)
            g = feat - mu[:, None]
            with torch.no_grad():
                k = self.match_cosine(g, unit, self.chunk)
            matched = unit[:, k]                                # [C, ..., N]
            matched = matched.movedim(0, -2) if k.ndim > 1 else matched
            p = (g * matched).sum(-2)
            return torch.mean(1 - p / torch.sqrt((g * g).sum(-2) + self.eps))
        with torch.no_grad():
            k = self.match(feat, self.target.to(feat.dtype), self.chunk)
        matched = self.target.to(feat.dtype)[:, k]              # [C, ..., N]
        matched = matched.movedim(0, -2) if k.ndim > 1 else matched
        return torch.mean((feat - matched) ** 2)


class StyleLossSliced(nn.Module):
    """The sliced Wasserstein loss (Heitz et al., "A Sliced Wasserstein Loss for Neural Texture Synthesis"): the W2 distance
    between the projections of the input's feature vectors and of a style tap's onto P random unit directions,
    ``mean_p,k (sort(R f)_p,k - T_p,k)^2`` with ``T = resample_N(sort_rows(R S))`` - ``StyleLossW2Marginal`` along random axes
    instead of the channel axes, so that over many forwards the whole C-dimensional distribution is matched.  Not in the
    reference; include/st_amd.h (st_plan_set_style_sliced) fixes the semantics: the directions and the sort are constants of the
    gradient, ties go by pixel index, there is no eps.  ``target`` = [C, M] (``get_target``), ``projections`` = P (None: C),
    ``seed``; ``epoch`` counts the direction sets drawn: with ``resample`` every forward in training mode uses the directions of
    the current epoch and advances it, otherwise (and in eval mode) the epoch stays.  ``directions``: None, or a [P, C] tensor to
    use instead of generated ones (``R = I`` gives StyleLossW2Marginal's value).  The torch path serves any device, dtype and
    batch, its directions drawn from a ``torch.Generator`` on the input's device; one dense fp32 HIP tensor whose channel count is
    a multiple of 64, with P a multiple of 64 in [64, 512], runs in the library, directions from the device generator (the two
    paths draw different, equally valid, directions)."""

    def __init__(self, target, projections=None, resample=True, seed=0):
        super().__init__()
        if target.ndim != 2:
            raise ValueError(f'target of shape {tuple(target.shape)}: [C, M], the style feature vectors as columns')
        if projections is not None and (not isinstance(projections, int) or isinstance(projections, bool) or projections < 1):
            raise ValueError(f'projections {projections!r}: None (the channel count), or an int >= 1')
        self.register_buffer('target', target)
        self.projections = int(projections) if projections is not None else int(target.shape[0])
        self.resample = bool(resample)
        self.seed = int(seed)
        self.epoch = 0
        self.directions = None

    @staticmethod
    def get_target(target):
        """The flattened features, [..., C, h w]: every pixel's feature vector as a column."""
        return target.flatten(-2)

    def draw(self, epoch, device, dtype=torch.float32):
        """The torch path's directions of ``epoch``: [P, C] standard normals from a generator on ``device`` seeded by (seed,
        epoch), every row divided by its norm."""
        gen = torch.Generator(device=device)
        gen.manual_seed((self.seed * 0x9e3779b1 + int(epoch) * 0x85ebca6b + 1) % (1 << 63))
        r = torch.randn((self.projections, self.target.shape[0]), generator=gen, device=device, dtype=torch.float32)
        return (r / r.norm(dim=1, keepdim=True)).to(dtype)

    def _native_ok(self, input):
        p = self.projections if self.directions is None else int(self.directions.shape[0])
        return (native.enabled and eligible(input, 'sliced') and self.target.shape[0] == input.shape[-3] and
                not self.target.requires_grad and self.target.device == input.device and self.target.dtype == torch.float32 and
                self.target.shape[1] <= _max_pixels() and 64 <= p <= 512 and p % 64 == 0 and
                (self.directions is None or (self.directions.device == input.device and self.directions.dtype == torch.float32 and
                                             not self.directions.requires_grad)))

    def forward(self, input):
        epoch = self.epoch
        if self.resample and self.training and self.directions is None:
            self.epoch += 1
        if self._native_ok(input):
            from . import _hip
            n = input.shape[-2] * input.shape[-1]
            target = self.target
            key = (epoch, n, target._version, None if self.directions is None else self.directions._version)
            cached = self.__dict__.get('_sliced_cache')
            if cached is None or cached[0] != key or cached[1] is not target or cached[2] is not self.directions:
                if self.directions is None:
                    r, rt = _hip.op_sliced_directions(self.seed, 0, epoch, self.projections, int(target.shape[0]), input.device)
                else:
                    r = self.directions.detach().contiguous()
                    rt = r.t().contiguous()
                t = _hip.op_sliced_target(target.contiguous(), r, rt, n)
                cached = self.__dict__['_sliced_cache'] = (key, target, self.directions, r, rt, t)
            return _SlicedLoss.apply(input, self, cached[3], cached[4], cached[5])
        r = self.directions if self.directions is not None else self.draw(epoch, input.device, input.dtype)
        return self._forward_torch(input, r)

    def _forward_torch(self, input, r):
        feat = input.flatten(-2)
        r = r.to(feat.dtype)
        n = feat.shape[-1]
        with torch.no_grad():
            q = torch.sort(r @ self.target.to(feat.dtype) + 0.0, dim=-1, stable=True).values
            target = StyleLossW2Marginal.resample(q, n)
        values = torch.sort(r @ feat + 0.0, dim=-1, stable=True).values
        return torch.mean((values - target) ** 2)


def _first_argmin(x, dim):
    """argmin along ``dim`` that returns the FIRST minimum (torch.argmin leaves the choice among equal values open)."""
    least = x.amin(dim=dim, keepdim=True)
    n = x.shape[dim]
    shape = [1] * x.ndim
    shape[dim] = n
    index = torch.arange(n, device=x.device).view(shape)
    return torch.where(x == least, index, n).amin(dim=dim)


class TVLoss(nn.Module):
    """L2 total variation over a nine-point stencil (reference :184-195; in the library: tv_interior_kernel)."""

    def forward(self, input):
        if native.enabled and eligible(input, 'tv'):
            return _TVLoss.apply(input, self)
        return self._forward_torch(input)

    def _forward_torch(self, input):
        x = F.pad(input, (1, 1, 1, 1), 'replicate')
        centre = x[..., 1:-1, 1:-1]
        right = (x[..., 1:-1, 2:] - centre).pow(2).mean() / 3
        down = (x[..., 2:, 1:-1] - centre).pow(2).mean() / 3
        diag_se = (x[..., 1:, 1:] - x[..., :-1, :-1]).pow(2).mean() / 12
        diag_sw = (x[..., 1:, :-1] - x[..., :-1, 1:]).pow(2).mean() / 12
        return 2 * (right + down + diag_se + diag_sw)


def laplacian(x):
    """The 4-neighbour Laplacian of a [..., h, w] map per channel, the map replicate-padded (as TVLoss pads the image):
    ``4 x[i][j] - x[i-][j] - x[i+][j] - x[i][j-] - x[i][j+]`` with the neighbour indices clamped to the map."""
    up = torch.cat([x[..., :1, :], x[..., :-1, :]], -2)
    down = torch.cat([x[..., 1:, :], x[..., -1:, :]], -2)
    left = torch.cat([x[..., :, :1], x[..., :, :-1]], -1)
    right = torch.cat([x[..., :, 1:], x[..., :, -1:]], -1)
    return 4 * x - up - down - left - right


def check_laplacian_pools(pools, height=None, width=None):
    """``pools`` as a tuple of 1 to 4 distinct positive integers, each - where a size is given - leaving a pooled map of at
    least 2 x 2 (on a 1-wide map the clamped Laplacian vanishes).  Raises ``ValueError``."""
    try:
        pools = tuple(pools)
    except TypeError:
        raise ValueError(f'pools {pools!r}: must be a sequence of 1 to 4 distinct positive integers') from None
    if not 1 <= len(pools) <= 4 or any(isinstance(p, bool) or not isinstance(p, int) or p < 1 for p in pools) or \
            len(set(pools)) != len(pools):
        raise ValueError(f'pools {pools!r}: must be 1 to 4 distinct positive integers')
    if height is not None:
        for p in pools:
            if height // p < 2 or width // p < 2:
                raise ValueError(f'pools {pools!r}: pool size {p} leaves a {height // p} x {width // p} map of the {height} x {width} '
                                 'image; the pooled map must be at least 2 x 2')
    return pools


class LaplacianLoss(nn.Module):
    """The Laplacian loss of Li et al., "Laplacian-Steered Neural Style Transfer", as this project fixes it (include/st_amd.h,
    st_plan_set_laplacian): the sum over ``pools`` - in list order - of ``mean((L(avg_pool2d(input, p)) - T_p) ** 2)`` with
    ``L`` the 4-neighbour Laplacian on the replicate-padded pooled map and ``T_p = L(avg_pool2d(content_image, p))``, a buffer.
    Not in the reference.  The torch path serves any device, dtype and batch; one dense fp32 HIP image runs in the library
    (lap_pool_kernel, lap_residual_kernel, lap_grad_kernel)."""

    def __init__(self, content_image, pools=(4,)):
        super().__init__()
        content_image = torch.as_tensor(content_image)
        if content_image.ndim < 3:
            raise ValueError(f'content image of shape {tuple(content_image.shape)}: must be [..., C, H, W]')
        self.pools = check_laplacian_pools(pools, *content_image.shape[-2:])
        with torch.no_grad():
            for k, p in enumerate(self.pools):
                self.register_buffer(f'target_{k}', self._laplacian_of(content_image.detach(), p))

    def extra_repr(self):
        return f'pools={self.pools}'

    @staticmethod
    def _laplacian_of(image, pool):
        if native.enabled and eligible(image, 'laplacian'):
            from . import _hip
            # the library's own kernels, so that the content image itself gives a residual of exactly 0 on the native path
            return _hip.op_laplacian_target(_dense(image), pool).view(image.shape[:-2] + (image.shape[-2] // pool, image.shape[-1] // pool))
        return laplacian(image if pool == 1 else F.avg_pool2d(image, pool))

    def targets(self):
        return [getattr(self, f'target_{k}') for k in range(len(self.pools))]

    def forward(self, input):
        targets = self.targets()
        if native.enabled and eligible(input, 'laplacian', targets):
            c, h, w = input.shape[-3:]
            # (one target per pool size, of that pool size's shape for THIS input, batch 1 or absent)
            if all(t.shape[-3:] == (c, h // p, w // p) and t.numel() == c * (h // p) * (w // p) for t, p in zip(targets, self.pools)):
                return _LaplacianLoss.apply(input, self, targets)
        return self._forward_torch(input)

    def _forward_torch(self, input):
        total = None
        for p, target in zip(self.pools, self.targets()):
            q = input if p == 1 else F.avg_pool2d(input, p)
            term = (laplacian(q) - target).pow(2).mean()
            total = term if total is None else total + term
        return total


class SumLoss(nn.ModuleList):
    """Sum of the member losses evaluated on the same arguments, on the last one's device (reference :198-208)."""

    def __init__(self, losses, verbose=False):
        super().__init__(losses)
        self.verbose = verbose

    def forward(self, *args, **kwargs):
        values = [member(*args, **kwargs) for member in self]
        if self.verbose:
            for i, value in enumerate(values):
                print(f'({i}): {value.item():g}')
        home = values[-1].device
        return sum(value.to(home) for value in values)


class Scale(nn.Module):
    """module(...) * scale (reference :211-221)."""

    def __init__(self, module, scale):
        super().__init__()
        self.module = module
        self.register_buffer('scale', torch.tensor(scale))

    def extra_repr(self):
        return f'(scale): {self.scale.item():g}'

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs) * self.scale


class LayerApply(nn.Module):
    """module(features[layer]) (reference :224-234)."""

    def __init__(self, module, layer):
        super().__init__()
        self.module = module
        self.layer = layer

    def extra_repr(self):
        return f'(layer): {self.layer!r}'

    def forward(self, input):
        return self.module(input[self.layer])

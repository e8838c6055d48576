"""Drop-in ``StyleTransfer`` / ``stylize()`` whose per-iteration hot path runs in libst_amd.so.

Mirrors the public surface of reference ``style_transfer/style_transfer.py:256-499`` (names, keyword-
only parameters, defaults, annotations, exceptions, callback protocol) so that ``cli.py`` - which
introspects ``stylize.__kwdefaults__`` / ``__annotations__`` (reference cli.py:150-153) - and user code
keep working.  What differs on purpose:

* the closure, Adam step, clamp and EMA update (reference :472-486) are ONE call into the HIP
  library per iteration (``Plan.step``); there is no autograd graph and no torchvision;
* devices must be HIP devices (PyTorch-ROCm names them ``cuda:N``).  There is no CPU path;
* the VGG-19 weights come from a user-supplied torchvision checkpoint (``vgg19-dcbb9e9d.pth``) or,
  for tests/benchmarks, from the seeded synthetic generator - this image has no network.

Python keeps only the cold path: the multi-scale pyramid, PIL resizing, target blending and the
scale-to-scale resampling of the optimiser state.
"""

import math
import operator
import os
import time
import warnings
from dataclasses import dataclass

import numpy as np
import torch
from PIL import Image
from torch.nn import functional as F

from . import _hip, losses, sqrtm, vgg  # noqa: F401  (sqrtm: importable as in the reference, :17)
# the reference defines its loss / bookkeeping modules in this file (:93-234); user code imports them from here
from .losses import (ContentLoss, ContentLossMSE, LayerApply, Scale, ScaledMSELoss, StyleLoss,  # noqa: F401
                     StyleLossW2, SumLoss, TVLoss, eye_like)

CONTENT_LAYERS = [22]
STYLE_LAYERS = [1, 6, 11, 20, 29]


# ---- small host helpers (reference :256-306) ---------------------------------------------------
def size_to_fit(size, max_dim, scale_up=False):
    """Fit (w, h) inside a max_dim square keeping aspect ratio (reference :256-265)."""
    w, h = size
    if not scale_up and max(h, w) <= max_dim:
        return w, h
    if h > w:
        return round(max_dim * w / h), max_dim
    return max_dim, round(max_dim * h / w)


def gen_scales(start, end):
    """end, end/sqrt2, end/2, ... down to >= start, ascending (reference :268-276)."""
    found, i, scale = set(), 0, end
    while scale >= start:
        found.add(scale)
        i += 1
        scale = round(end / pow(2, i / 2))
    return sorted(found)


def interpolate(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        return F.interpolate(*args, **kwargs)


def scale_adam(state, shape):
    """A torch.optim.Adam ``state_dict()`` resampled to a new image size - the warm start of the next scale
    (reference :285-295): first moments bicubic, second moments (and amsgrad's running maximum) bilinear and
    clipped at zero, the step count kept.  stylize() itself keeps its Adam state in AdamState (the fused HIP step
    owns the update); this function serves user code that drives a torch optimiser the reference's way."""
    import copy
    out = copy.deepcopy(state)
    for entry in out['state'].values():
        entry['exp_avg'] = interpolate(entry['exp_avg'], shape, mode='bicubic')
        for key in ('exp_avg_sq', 'max_exp_avg_sq'):
            if key in entry:
                entry[key] = interpolate(entry[key], shape, mode='bilinear').relu_()
    return out


def to_tensor(pil_image):
    """PIL RGB -> float CHW in [0,1] (what torchvision's TF.to_tensor does for uint8 images)."""
    arr = np.asarray(pil_image.convert('RGB'), dtype=np.uint8)
    return torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def to_pil_image(tensor):
    """float CHW in [0,1] -> PIL RGB; mul(255).byte() truncation like torchvision's to_pil_image."""
    arr = tensor.detach().cpu().mul(255).byte().permute(1, 2, 0).numpy()
    return Image.fromarray(arr, 'RGB')


@dataclass
class STIterate:
    w: int
    h: int
    i: int
    i_max: int
    loss: float
    time: float
    gpu_ram: int


class EMA:
    """Bias-corrected exponential moving average of the iterates (reference :237-253).

    ``value`` lives on the device and is advanced inside the fused HIP step; ``accum`` and ``decay``
    are fp32 scalars kept on the host with the same fp32 arithmetic as the reference's buffers."""

    def __init__(self, input, decay):
        self.value = torch.zeros_like(input)
        self.decay = torch.tensor(decay, dtype=torch.float32)
        self.accum = torch.tensor(1., dtype=torch.float32)
        self.update(input)

    def get(self):
        return self.value / (1 - self.accum).to(self.value.device)

    def advance_accum(self):
        self.accum = self.accum * self.decay

    def update(self, input):
        self.advance_accum()
        d = self.decay.to(self.value.device)
        self.value *= d
        self.value += (1 - d) * input.detach()


class AdamState:
    """exp_avg / exp_avg_sq / step of torch.optim.Adam for the single image tensor."""

    def __init__(self, image):
        self.exp_avg = torch.zeros_like(image)
        self.exp_avg_sq = torch.zeros_like(image)
        self.step = 0

    def rescaled(self, shape):
        """Warm start at a new scale (reference scale_adam, :285-295): moments resampled, step kept."""
        new = AdamState.__new__(AdamState)
        new.exp_avg = interpolate(self.exp_avg, shape, mode='bicubic').contiguous()
        new.exp_avg_sq = interpolate(self.exp_avg_sq, shape, mode='bilinear').relu_().contiguous()
        new.step = self.step
        return new


def _dist_info():
    """(rank, world) of the default torch.distributed group; (0, 1) when not initialised."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _gather_rows(strip, rows, rank):
    """Full [1, C, H, W] tensor on EVERY rank from the ranks' row strips (cold path: once per scale).
    One broadcast per rank, because the strips have different heights."""
    import torch.distributed as dist
    parts = []
    for r, (b, e) in enumerate(rows):
        buf = strip.contiguous() if r == rank else strip.new_empty((strip.shape[0], strip.shape[1], e - b, strip.shape[3]))
        if strip.is_cuda:
            torch.cuda.synchronize(strip.device)          # gloo on device tensors is not stream-ordered
        dist.broadcast(buf, src=r)
        parts.append(buf)
    return torch.cat(parts, dim=2)


def _starting_image(init, content_image, style_images, style_weights, height, width):
    """The iterate the first scale starts from, [1, 3, height, width] on the host (reference style_transfer.py:380-406).
    The random modes draw from torch's global generator in the reference's order and with its calls, so that
    torch.manual_seed(n) (the CLI's --random-seed) reproduces the reference's starting point draw for draw:
    'gray' one rand of the full shape, 'uniform' the same, 'normal' one trunc_normal_ of the full shape,
    'style_stats' one trunc_normal_ per colour channel (R, G, B in turn)."""
    shape = [1, 3, height, width]
    if init == 'content':
        return to_tensor(content_image.resize((width, height), Image.BICUBIC))[None]
    if init == 'gray':                                        # mid-gray plus at most one 8-bit step of noise
        return torch.rand(shape) / 255 + 0.5
    if init == 'uniform':
        return torch.rand(shape)
    if init == 'normal':
        out = torch.empty(shape)
        torch.nn.init.trunc_normal_(out, mean=0.5, std=0.25, a=0, b=1)
        return out
    if init == 'style_stats':
        # per-channel mean and (unbiased) variance of every style image, blended with the style weights
        blend_mean, blend_var = torch.zeros(3), torch.zeros(3)
        for pil, weight in zip(style_images, style_weights):
            pixels = to_tensor(pil)
            blend_mean = blend_mean + pixels.mean(dim=(1, 2)) * weight
            blend_var = blend_var + pixels.var(dim=(1, 2)) * weight
        planes = []
        for c in range(3):
            plane = torch.empty([1, 1, height, width])
            torch.nn.init.trunc_normal_(plane, mean=blend_mean[c], std=blend_var[c].sqrt(), a=0, b=1)
            planes.append(plane)
        return torch.cat(planes, dim=1)
    raise ValueError("init must be one of 'content', 'gray', 'uniform', 'style_mean'")


def _resolve_taps(content_layers, style_layers, style_weights, world=1):
    """``StyleTransfer.content_layers`` / ``style_layers`` / ``style_weights`` as the fused closure takes them: returns
    (content layers, style layers, their weights).  The style pairs are ``zip(style_layers, style_weights)`` as the reference
    forms them (:451).  Raises ``ValueError`` for what the closure cannot serve, before any device work."""
    content = [int(layer) for layer in content_layers]
    pairs = [(int(layer), float(weight)) for layer, weight in zip(style_layers, style_weights)]
    style = [layer for layer, _ in pairs]
    for name, layers in (('content_layers', content), ('style_layers', style)):
        for layer in layers:
            if layer not in _hip.TAPS:
                raise ValueError(
                    f'{name}: features[{layer}] is not one of the 17 taps of the fused trunk - the ReLU outputs 1, 3, 6, 8, 11, '
                    '13, 15, 17, 20, 22, 24, 26, 29 and the pool outputs 4, 9, 18, 27.  The pre-ReLU convolution outputs, which '
                    'the reference accepts, are not kept by the fused trunk.')
        if len(set(layers)) != len(layers):
            raise ValueError(f'{name}: a layer is named twice in {layers}')
        if len(layers) > 16:
            raise ValueError(f'{name}: {len(layers)} layers; the fused closure takes at most 16 per list')
    if not content and not style:
        raise ValueError('content_layers and style_layers are both empty')
    default = (tuple(content), tuple(style)) == (_hip.DEFAULT_CONTENT_LAYERS, _hip.DEFAULT_STYLE_LAYERS)
    if world > 1 and not default:
        raise ValueError(f'content_layers {content} / style_layers {style} on {world} ranks: row strips run the default layers '
                         '(content [22], style [1, 6, 11, 20, 29]) only; other layer sets are out of scope for strips - run '
                         'them on one device')
    return content, style, [weight for _, weight in pairs]


def _resolve_loss_kinds(content_loss, style_loss, world=1):
    """``StyleTransfer.content_loss`` / ``style_loss`` as the fused closure takes them: returns the two names.  Raises
    ``ValueError`` for an unknown name and for a non-default kind on several ranks, before any device work."""
    if content_loss not in _hip.CONTENT_LOSSES:
        raise ValueError(f'content_loss {content_loss!r}: must be one of {list(_hip.CONTENT_LOSSES)} '
                         "('mse': ContentLossMSE, 'scaled_mse': ContentLoss)")
    if style_loss not in _hip.STYLE_LOSSES:
        raise ValueError(f'style_loss {style_loss!r}: must be one of {list(_hip.STYLE_LOSSES)} '
                         "('w2': StyleLossW2, 'gram': StyleLoss on Gram matrices)")
    default = (content_loss, style_loss) == (_hip.CONTENT_LOSSES[0], _hip.STYLE_LOSSES[0])
    if world > 1 and not default:
        raise ValueError(f'content_loss {content_loss!r} / style_loss {style_loss!r} on {world} ranks: row strips run the '
                         "default kinds ('mse', 'w2') only; other loss kinds are out of scope for strips - run them on one "
                         'device')
    return content_loss, style_loss


# the eps of each kind's module as the reference's constructors default it (StyleLossW2 :152, StyleLoss :130, ContentLoss :110)
_LOSS_EPS = {'w2': 1e-4, 'gram': 1e-8, 'scaled_mse': 1e-8}


def _resolve_layer_losses(content_loss, style_loss, content_eps, style_eps, n_content, n_style, world=1):
    """``StyleTransfer.content_loss`` / ``style_loss`` / ``content_eps`` / ``style_eps`` per LAYER, as the fused closure takes
    them: returns (content kinds, style kinds, content eps, style eps), one entry per layer of the list, an eps None where
    the layer has its kind's default.  A kind is a name - every layer of the list - or a sequence with one name per layer;
    an eps is None, a number - every layer - or a sequence of None / number per layer.  Raises ``ValueError`` naming the
    attribute for a wrong length, an unknown name, an eps on an 'mse' layer, a negative or non-finite eps, and for any
    non-default entry on several ranks, before any device work."""
    kinds = []
    for attr, given, n in (('content_loss', content_loss, n_content), ('style_loss', style_loss, n_style)):
        single = not isinstance(given, (list, tuple))        # (anything else is taken as ONE name, and refused as unknown)
        names = [given] * n if single else list(given)
        if len(names) != n:
            raise ValueError(f'{attr} {given!r}: {len(names)} names for {n} layers; give one name, or exactly one per entry '
                             f'of {attr.split("_")[0]}_layers')
        for name in names if names or not single else [given]:
            # (the unknown-name messages are _resolve_loss_kinds')
            _resolve_loss_kinds(*((name, _hip.STYLE_LOSSES[0]) if attr == 'content_loss' else (_hip.CONTENT_LOSSES[0], name)))
        kinds.append(names)
    epses = []
    for attr, given, names in (('content_eps', content_eps, kinds[0]), ('style_eps', style_eps, kinds[1])):
        values = [given] * len(names) if given is None or isinstance(given, (int, float)) else list(given)
        if len(values) != len(names):
            raise ValueError(f'{attr} {given!r}: {len(values)} values for {len(names)} layers; give None, one number, or '
                             f'exactly one (None for the default) per entry of {attr.split("_")[0]}_layers')
        for i, (value, name) in enumerate(zip(values, names)):
            if value is None:
                continue
            if isinstance(value, str) or not math.isfinite(value) or value < 0:
                raise ValueError(f'{attr} {given!r}: {value!r} is not a finite non-negative number (None: the default)')
            if name not in _LOSS_EPS:
                raise ValueError(f"{attr} {given!r}: layer {i} has the loss {name!r} (ContentLossMSE), which has no eps; "
                                 'give None for it')
            # (the library's eps is a float: a number that IS the default there counts as the default)
            values[i] = None if np.float32(value) == np.float32(_LOSS_EPS[name]) else float(value)
        epses.append(values)
    default = (all(name == _hip.CONTENT_LOSSES[0] for name in kinds[0]) and all(name == _hip.STYLE_LOSSES[0] for name in kinds[1])
               and all(value is None for value in epses[0] + epses[1]))
    if world > 1 and not default:
        raise ValueError(f'content_loss {content_loss!r} / style_loss {style_loss!r} / content_eps {content_eps!r} / style_eps '
                         f"{style_eps!r} on {world} ranks: row strips run the default kinds ('mse', 'w2') with their default eps "
                         'only; other loss kinds are out of scope for strips - run them on one device')
    return kinds[0], kinds[1], epses[0], epses[1]


def _resolve_style_diagonal(style_diagonal, style_loss, world=1):
    """``StyleTransfer.style_diagonal`` as the fused closure takes it: one bool per entry of ``style_loss`` (the resolved
    kinds, one per style layer).  A bool means every 'w2' layer; a sequence holds one bool per entry of style_layers.  Raises
    ``ValueError`` naming the attribute for a wrong length, a value that is no bool, a true flag on a 'gram' layer, and for
    any true flag on several ranks, before any device work."""
    n = len(style_loss)
    if isinstance(style_diagonal, (bool, np.bool_)):
        flags = [bool(style_diagonal) and name == _hip.STYLE_LOSSES[0] for name in style_loss]
    else:
        if isinstance(style_diagonal, str) or not isinstance(style_diagonal, (list, tuple)):
            raise ValueError(f'style_diagonal {style_diagonal!r}: give a bool, or a sequence with one bool per entry of style_layers')
        flags = list(style_diagonal)
        if len(flags) != n:
            raise ValueError(f'style_diagonal {style_diagonal!r}: {len(flags)} flags for {n} layers; give one bool, or exactly '
                             'one per entry of style_layers')
        for i, (flag, name) in enumerate(zip(flags, style_loss)):
            if not isinstance(flag, (bool, np.bool_)) and flag not in (0, 1):
                raise ValueError(f'style_diagonal {style_diagonal!r}: {flag!r} is not a bool')
            if flag and name != _hip.STYLE_LOSSES[0]:
                raise ValueError(f"style_diagonal {style_diagonal!r}: layer {i} has the loss {name!r} (StyleLoss on Gram "
                                 "matrices); only a 'w2' layer's covariances can be restricted to their diagonals")
        flags = [bool(flag) for flag in flags]
    if world > 1 and any(flags):
        raise ValueError(f'style_diagonal {style_diagonal!r} on {world} ranks: row strips run full W2 heads only; diagonal '
                         'heads are out of scope for strips - run them on one device')
    return flags


def _resolve_style_marginal(style_marginal, style_loss, style_diagonal=None, style_eps=None, masked=False, world=1):
    """``StyleTransfer.style_marginal`` as the fused closure takes it: one bool per entry of ``style_loss`` (the resolved
    kinds).  A bool means every 'w2' layer that is not flagged diagonal; a sequence holds one bool per entry of style_layers.
    ``style_diagonal`` / ``style_eps``: the resolved lists (one per layer, eps None = default).  Raises ``ValueError``
    naming the attribute for a wrong length, a value that is no bool, a true flag on a 'gram' layer, on a layer flagged
    diagonal or with a custom eps, for any true flag together with style masks or regions (``masked``) or on several
    ranks, before any device work."""
    n = len(style_loss)
    diagonal = list(style_diagonal) if style_diagonal is not None else [False] * n
    epses = list(style_eps) if style_eps is not None else [None] * n
    if isinstance(style_marginal, (bool, np.bool_)):
        flags = [bool(style_marginal) and name == _hip.STYLE_LOSSES[0] and not diag for name, diag in zip(style_loss, diagonal)]
    else:
        if isinstance(style_marginal, str) or not isinstance(style_marginal, (list, tuple)):
            raise ValueError(f'style_marginal {style_marginal!r}: give a bool, or a sequence with one bool per entry of style_layers')
        flags = list(style_marginal)
        if len(flags) != n:
            raise ValueError(f'style_marginal {style_marginal!r}: {len(flags)} flags for {n} layers; give one bool, or exactly '
                             'one per entry of style_layers')
        for i, (flag, name) in enumerate(zip(flags, style_loss)):
            if not isinstance(flag, (bool, np.bool_)) and flag not in (0, 1):
                raise ValueError(f'style_marginal {style_marginal!r}: {flag!r} is not a bool')
            if flag and name != _hip.STYLE_LOSSES[0]:
                raise ValueError(f"style_marginal {style_marginal!r}: layer {i} has the loss {name!r} (StyleLoss on Gram "
                                 "matrices); only a 'w2' layer can be matched on its marginals")
            if flag and diagonal[i]:
                raise ValueError(f'style_marginal {style_marginal!r}: layer {i} is flagged in style_diagonal too; a layer takes '
                                 'one of the two')
        flags = [bool(flag) for flag in flags]
    for i, flag in enumerate(flags):
        if flag and epses[i] is not None:
            raise ValueError(f'style_marginal {style_marginal!r}: layer {i} has the custom style_eps {epses[i]!r}; the marginal '
                             'term has no eps')
    if masked and any(flags):
        raise ValueError(f'style_marginal {style_marginal!r} together with style_mask, style_regions or style_image_masks: '
                         'weighted quantiles are out of scope - clear one of them')
    if world > 1 and any(flags):
        raise ValueError(f'style_marginal {style_marginal!r} on {world} ranks: row strips run full W2 heads only; marginal '
                         'heads are out of scope for strips - run them on one device')
    return flags


def _resolve_style_nearest(style_nearest, style_loss, style_diagonal=None, style_marginal=None, style_eps=None, masked=False,
                           world=1, samples=None):
    """``StyleTransfer.style_nearest`` as the fused closure takes it: one bool per entry of ``style_loss`` (the resolved
    kinds).  A bool means every 'w2' layer that is flagged neither diagonal nor marginal; a sequence holds one bool per entry
    of style_layers.  ``style_diagonal`` / ``style_marginal`` / ``style_eps``: the resolved lists (one per layer, eps None =
    default).  ``samples``: ``StyleTransfer.style_nearest_samples``, checked here too.  Raises ``ValueError`` naming the
    attribute for a wrong length, a value that is no bool, a true flag on a 'gram' layer, on a layer flagged diagonal or
    marginal or with a custom eps, for any true flag together with style masks or regions (``masked``) or on several ranks,
    and for ``style_nearest_samples`` that is neither None nor an int >= 1, before any device work."""
    if samples is not None and (isinstance(samples, (bool, np.bool_)) or not isinstance(samples, (int, np.integer)) or samples < 1):
        raise ValueError(f'style_nearest_samples {samples!r}: None, or an int >= 1 (the style vectors kept per layer and image)')
    n = len(style_loss)
    diagonal = list(style_diagonal) if style_diagonal is not None else [False] * n
    marginal = list(style_marginal) if style_marginal is not None else [False] * n
    epses = list(style_eps) if style_eps is not None else [None] * n
    if isinstance(style_nearest, (bool, np.bool_)):
        flags = [bool(style_nearest) and name == _hip.STYLE_LOSSES[0] and not diag and not marg
                 for name, diag, marg in zip(style_loss, diagonal, marginal)]
    else:
        if isinstance(style_nearest, str) or not isinstance(style_nearest, (list, tuple)):
            raise ValueError(f'style_nearest {style_nearest!r}: give a bool, or a sequence with one bool per entry of style_layers')
        flags = list(style_nearest)
        if len(flags) != n:
            raise ValueError(f'style_nearest {style_nearest!r}: {len(flags)} flags for {n} layers; give one bool, or exactly '
                             'one per entry of style_layers')
        for i, (flag, name) in enumerate(zip(flags, style_loss)):
            if not isinstance(flag, (bool, np.bool_)) and flag not in (0, 1):
                raise ValueError(f'style_nearest {style_nearest!r}: {flag!r} is not a bool')
            if flag and name != _hip.STYLE_LOSSES[0]:
                raise ValueError(f"style_nearest {style_nearest!r}: layer {i} has the loss {name!r} (StyleLoss on Gram "
                                 "matrices); only a 'w2' layer can be matched on nearest style vectors")
            if flag and diagonal[i]:
                raise ValueError(f'style_nearest {style_nearest!r}: layer {i} is flagged in style_diagonal too; a layer takes '
                                 'one of the two')
            if flag and marginal[i]:
                raise ValueError(f'style_nearest {style_nearest!r}: layer {i} is flagged in style_marginal too; a layer takes '
                                 'one of the two')
        flags = [bool(flag) for flag in flags]
    for i, flag in enumerate(flags):
        if flag and epses[i] is not None:
            raise ValueError(f'style_nearest {style_nearest!r}: layer {i} has the custom style_eps {epses[i]!r}; the nearest '
                             'term has no eps')
    if masked and any(flags):
        raise ValueError(f'style_nearest {style_nearest!r} together with style_mask, style_regions or style_image_masks: '
                         'masked matching is out of scope - clear one of them')
    if world > 1 and any(flags):
        raise ValueError(f'style_nearest {style_nearest!r} on {world} ranks: row strips run full W2 heads only; nearest '
                         'heads are out of scope for strips - run them on one device')
    return flags


def _resolve_style_nearest_metric(style_nearest_metric, style_nearest, world=1):
    """``StyleTransfer.style_nearest_metric`` as the fused closure takes it: one name of ``_hip.NEAREST_METRICS`` per entry of
    ``style_nearest`` (the resolved flags).  A name means that metric on every flagged layer ('l2' on the others); a sequence
    holds one name per entry of style_layers.  Raises ``ValueError`` naming the attribute for a wrong length, an unknown name,
    a name other than 'l2' on a layer that is not flagged, and for a metric other than 'l2' on several ranks, before any device
    work."""
    names, n = _hip.NEAREST_METRICS, len(style_nearest)
    if isinstance(style_nearest_metric, str):
        if style_nearest_metric not in names:
            raise ValueError(f'style_nearest_metric {style_nearest_metric!r}: one of {names}')
        metrics = [style_nearest_metric if flag else names[0] for flag in style_nearest]
    else:
        if not isinstance(style_nearest_metric, (list, tuple)):
            raise ValueError(f'style_nearest_metric {style_nearest_metric!r}: give one of {names}, or a sequence with one name per '
                             'entry of style_layers')
        metrics = list(style_nearest_metric)
        if len(metrics) != n:
            raise ValueError(f'style_nearest_metric {style_nearest_metric!r}: {len(metrics)} names for {n} layers; give one name, '
                             'or exactly one per entry of style_layers')
        for i, (name, flag) in enumerate(zip(metrics, style_nearest)):
            if not isinstance(name, str) or name not in names:
                raise ValueError(f'style_nearest_metric {style_nearest_metric!r}: {name!r} is none of {names}')
            if name != names[0] and not flag:
                raise ValueError(f'style_nearest_metric {style_nearest_metric!r}: layer {i} is not flagged in style_nearest; only '
                                 f'a layer matched on nearest style vectors takes the metric {name!r}')
    if world > 1 and any(name != names[0] for name in metrics):
        raise ValueError(f'style_nearest_metric {style_nearest_metric!r} on {world} ranks: nearest heads are out of scope for '
                         'strips - run them on one device')
    return metrics


def _resolve_style_sliced(style_sliced, style_loss, style_diagonal=None, style_marginal=None, style_nearest=None, style_eps=None,
                          masked=False, world=1, projections=None, samples=None, resample=True, seed=0, optimizer='adam'):
    """``StyleTransfer.style_sliced`` as the fused closure takes it: one bool per entry of ``style_loss`` (the resolved kinds).
    A bool means every 'w2' layer that is flagged neither diagonal, marginal nor nearest; a sequence holds one bool per entry
    of style_layers.  ``style_diagonal`` / ``style_marginal`` / ``style_nearest`` / ``style_eps``: the resolved lists (one per
    layer, eps None = default).  ``projections`` / ``samples`` / ``resample`` / ``seed``: ``StyleTransfer.style_sliced_projections``
    / ``_samples`` / ``_resample`` / ``_seed``, checked here too.  Raises ``ValueError`` naming the attribute for a wrong length,
    a value that is no bool, a true flag on a 'gram' layer, on a layer flagged diagonal, marginal or nearest or with a custom
    eps, for any true flag together with style masks or regions (``masked``) or on several ranks, for projections that are
    neither None nor a multiple of 64 in [64, 512], samples that are neither None nor an int >= 1, a resample that is no bool,
    a seed that is no int >= 0, and for ``optimizer='lbfgs'`` with resampling on, before any device work."""
    def is_int(value):
        return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_))
    if projections is not None and (not is_int(projections) or projections < 64 or projections > 512 or projections % 64):
        raise ValueError(f'style_sliced_projections {projections!r}: None (the layer\'s channel count), or a multiple of 64 in [64, 512]')
    if samples is not None and (not is_int(samples) or samples < 1):
        raise ValueError(f'style_sliced_samples {samples!r}: None, or an int >= 1 (the style vectors kept per layer and image)')
    if not isinstance(resample, (bool, np.bool_)):
        raise ValueError(f'style_sliced_resample {resample!r}: a bool')
    if not is_int(seed) or seed < 0 or seed >= 1 << 64:
        raise ValueError(f'style_sliced_seed {seed!r}: an int in [0, 2^64)')
    n = len(style_loss)
    diagonal = list(style_diagonal) if style_diagonal is not None else [False] * n
    marginal = list(style_marginal) if style_marginal is not None else [False] * n
    nearest = list(style_nearest) if style_nearest is not None else [False] * n
    epses = list(style_eps) if style_eps is not None else [None] * n
    if isinstance(style_sliced, (bool, np.bool_)):
        flags = [bool(style_sliced) and name == _hip.STYLE_LOSSES[0] and not diag and not marg and not near
                 for name, diag, marg, near in zip(style_loss, diagonal, marginal, nearest)]
    else:
        if isinstance(style_sliced, str) or not isinstance(style_sliced, (list, tuple)):
            raise ValueError(f'style_sliced {style_sliced!r}: give a bool, or a sequence with one bool per entry of style_layers')
        flags = list(style_sliced)
        if len(flags) != n:
            raise ValueError(f'style_sliced {style_sliced!r}: {len(flags)} flags for {n} layers; give one bool, or exactly '
                             'one per entry of style_layers')
        for i, (flag, name) in enumerate(zip(flags, style_loss)):
            if not isinstance(flag, (bool, np.bool_)) and flag not in (0, 1):
                raise ValueError(f'style_sliced {style_sliced!r}: {flag!r} is not a bool')
            if flag and name != _hip.STYLE_LOSSES[0]:
                raise ValueError(f"style_sliced {style_sliced!r}: layer {i} has the loss {name!r} (StyleLoss on Gram "
                                 "matrices); only a 'w2' layer can be matched on sliced projections")
            for other, attr in ((diagonal, 'style_diagonal'), (marginal, 'style_marginal'), (nearest, 'style_nearest')):
                if flag and other[i]:
                    raise ValueError(f'style_sliced {style_sliced!r}: layer {i} is flagged in {attr} too; a layer takes one of the two')
        flags = [bool(flag) for flag in flags]
    for i, flag in enumerate(flags):
        if flag and epses[i] is not None:
            raise ValueError(f'style_sliced {style_sliced!r}: layer {i} has the custom style_eps {epses[i]!r}; the sliced '
                             'term has no eps')
    if masked and any(flags):
        raise ValueError(f'style_sliced {style_sliced!r} together with style_mask, style_regions or style_image_masks: '
                         'weighted quantiles are out of scope - clear one of them')
    if world > 1 and any(flags):
        raise ValueError(f'style_sliced {style_sliced!r} on {world} ranks: row strips run full W2 heads only; sliced '
                         'heads are out of scope for strips - run them on one device')
    if any(flags) and resample and optimizer == 'lbfgs':
        raise ValueError("style_sliced with style_sliced_resample=True and optimizer='lbfgs': L-BFGS's history assumes one "
                         'objective, and new directions at every evaluation change it - set style_sliced_resample = False')
    return flags


def _nearest_sample_columns(m, samples):
    """The columns of a style tap of m pixels that ``style_nearest_samples`` keeps: all of them, or ``floor(t m / K)``,
    t = 0 ... K - 1, when m > K."""
    if samples is None or m <= samples:
        return list(range(m))
    return [(t * m) // samples for t in range(samples)]


def _mask_image(mask, attr):
    """One mask as (PIL image, divisor): a PIL image becomes mode 'L' (divisor 255), a 2-D numpy / torch array with values
    in [0, 1] a mode 'F' image (divisor 1).  Raises ``ValueError`` naming ``attr``."""
    if isinstance(mask, Image.Image):
        image = mask.convert('L')
        if image.getextrema()[1] == 0:
            raise ValueError(f'{attr}: the mask is zero everywhere; no pixel would carry the style statistics')
        return image, 255.0
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    try:
        values = np.asarray(mask, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f'{attr}: a mask is a PIL image or a 2-D numpy / torch array, not {type(mask).__name__}') from None
    if values.ndim != 2 or values.size == 0:
        raise ValueError(f'{attr}: a mask array has 2 dimensions (height, width), not shape {tuple(values.shape)}')
    if not np.isfinite(values).all() or values.min() < 0 or values.max() > 1:
        raise ValueError(f'{attr}: the mask holds non-finite values or values outside [0, 1]')
    if values.max() == 0:
        raise ValueError(f'{attr}: the mask is zero everywhere; no pixel would carry the style statistics')
    return Image.fromarray(np.ascontiguousarray(values), mode='F'), 1.0


def _resolve_style_masks(style_mask, style_image_masks, n_style_images, world=1):
    """``StyleTransfer.style_mask`` / ``style_image_masks`` as stylize() takes them: returns (the output mask or None, one
    entry - a mask or None - per style image), every mask as ``_mask_image`` gives it, for ``_sized_mask`` to bring to a
    scale's size.  Raises ``ValueError`` naming the attribute for a list of the wrong length, an array of the wrong number
    of dimensions, values outside [0, 1] or non-finite, an all-zero mask, and for any mask on several ranks, before any
    device work."""
    output = None if style_mask is None else _mask_image(style_mask, 'style_mask')
    if style_image_masks is None:
        per_image = [None] * n_style_images
    else:
        if isinstance(style_image_masks, (Image.Image, np.ndarray, torch.Tensor)) or not hasattr(style_image_masks, '__len__'):
            raise ValueError('style_image_masks: give None, or a list with exactly one entry (None or a mask) per style image')
        if len(style_image_masks) != n_style_images:
            raise ValueError(f'style_image_masks: {len(style_image_masks)} entries for {n_style_images} style images; give '
                             'None, or exactly one entry (None or a mask) per style image')
        per_image = [None if mask is None else _mask_image(mask, f'style_image_masks[{i}]')
                     for i, mask in enumerate(style_image_masks)]
    if world > 1 and (output is not None or any(entry is not None for entry in per_image)):
        raise ValueError(f'style_mask / style_image_masks on {world} ranks: row strips take no style mask (a level\'s sum would '
                         'span the ranks); masks are out of scope for strips - run them on one device')
    return output, per_image


def _resolve_weight_maps(content_mask, tv_mask, world=1):
    """``StyleTransfer.content_mask`` / ``tv_mask`` as stylize() takes them: (the content map or None, the TV map or None), each
    as ``_mask_image`` gives it, for ``_sized_mask`` to bring to a scale's size.  Raises ``ValueError`` naming the attribute for
    an array of the wrong number of dimensions, values outside [0, 1] or non-finite, an all-zero map, and for either map on
    several ranks, before any device work."""
    maps = []
    for attr, mask in (('content_mask', content_mask), ('tv_mask', tv_mask)):
        if mask is None:
            maps.append(None)
            continue
        try:
            maps.append(_mask_image(mask, attr))
        except ValueError as exc:
            # (_mask_image words an all-zero mask for the style statistics)
            raise ValueError(str(exc).replace('; no pixel would carry the style statistics', '; the term would vanish everywhere')) from None
        if world > 1:
            raise ValueError(f'{attr} on {world} ranks: row strips take no content or TV map (the general closure serves them); '
                             'maps are out of scope for strips - run them on one device')
    return tuple(maps)


def _resolve_laplacian(laplacian_weight, laplacian_pools, height=None, width=None, world=1):
    """``StyleTransfer.laplacian_weight`` / ``laplacian_pools`` as stylize() takes them: None for a weight of 0 (no term, the
    setter is not called), else (weight, pools) for ``Plan.set_laplacian``.  ``height`` x ``width`` is the SMALLEST scale's image
    (None: no size to check): a pool size that leaves it a 2 x 2 map leaves every scale one.  Raises ``ValueError`` naming the attribute for a negative
    or non-finite weight, pools that are not 1 to 4 distinct positive integers, a pool too large for that image, and for a
    non-zero weight on several ranks, before any device work."""
    try:
        weight = float(laplacian_weight)
    except (TypeError, ValueError):
        raise ValueError(f'laplacian_weight {laplacian_weight!r}: must be a number >= 0') from None
    if not math.isfinite(weight) or weight < 0:
        raise ValueError(f'laplacian_weight {laplacian_weight!r}: must be finite and >= 0 (0: no Laplacian term)')
    try:
        pools = losses.check_laplacian_pools(laplacian_pools)
        if weight > 0:
            losses.check_laplacian_pools(pools, height, width)
    except ValueError as exc:
        detail = str(exc).split(': ', 1)[1]
        raise ValueError(f'laplacian_pools {laplacian_pools!r}: {detail}' + (
            ' at the smallest scale' if 'leaves' in detail else '')) from None
    if weight == 0:
        return None
    if world > 1:
        raise ValueError(f'laplacian_weight {weight:g} on {world} ranks: row strips take no Laplacian term (the general closure '
                         'serves it); it is out of scope for strips - run it on one device')
    return weight, pools


MAX_STYLE_REGIONS = 4


def _resolve_style_regions(style_regions, style_image_regions, style_region_weights, n_style_images, style_weights=None,
                           style_mask=None, world=1):
    """``StyleTransfer.style_regions`` / ``style_image_regions`` / ``style_region_weights`` as stylize() takes them: None, or
    (one mask per region as ``_mask_image`` gives it, the region index of every style image, the regions' weights or None).
    ``style_weights``: stylize()'s argument as given (None: equal weights) - a region's target blends its own images' moments
    with ``style_weights[i]`` over the region's sum, which must not be 0.  Raises ``ValueError`` naming the attribute -
    a wrong length, an index out of range, a region without an image or whose images' weights sum to 0, more than 4 regions,
    ``style_mask`` together with ``style_regions``, weights that are not finite and non-negative with one positive, and any
    region on several ranks - before any device work."""
    if style_regions is None:
        if style_image_regions is not None or style_region_weights is not None:
            raise ValueError('style_image_regions / style_region_weights: given without style_regions')
        return None
    if isinstance(style_regions, (Image.Image, np.ndarray, torch.Tensor)) or not hasattr(style_regions, '__len__'):
        raise ValueError('style_regions: give None, or a list of 1 to 4 masks, one per region')
    count = len(style_regions)
    if not 1 <= count <= MAX_STYLE_REGIONS:
        raise ValueError(f'style_regions: {count} regions; a plan takes 1 to {MAX_STYLE_REGIONS}')
    if style_mask is not None:
        raise ValueError('style_mask together with style_regions: a plan takes one or the other (a single region IS a style mask)')
    if world > 1:
        raise ValueError(f'style_regions on {world} ranks: row strips take no style regions (a level\'s sum would span the '
                         'ranks); regions are out of scope for strips - run them on one device')
    regions = [_mask_image(mask, f'style_regions[{r}]') for r, mask in enumerate(style_regions)]
    if style_image_regions is None:
        raise ValueError('style_image_regions: required with style_regions - one region index per style image')
    try:
        image_regions = [operator.index(r) for r in style_image_regions]
    except TypeError:
        raise ValueError('style_image_regions: one integer region index per style image') from None
    if len(image_regions) != n_style_images:
        raise ValueError(f'style_image_regions: {len(image_regions)} entries for {n_style_images} style images; give exactly one '
                         'region index per style image')
    for i, r in enumerate(image_regions):
        if not 0 <= r < count:
            raise ValueError(f'style_image_regions[{i}]: region {r} out of range (0 .. {count - 1})')
    image_weights = [1.0] * n_style_images if style_weights is None else [float(w) for w in style_weights]
    for r in range(count):
        own = [i for i, region in enumerate(image_regions) if region == r]
        if not own:
            raise ValueError(f'style_image_regions: region {r} has no style image')
        if len(image_weights) == n_style_images and sum(image_weights[i] for i in own) == 0:
            raise ValueError(f'style_image_regions: the style_weights of region {r}\'s images sum to 0')
    weights = None
    if style_region_weights is not None:
        try:
            weights = [float(w) for w in style_region_weights]
        except TypeError:
            raise ValueError('style_region_weights: give None, or one number per region') from None
        if len(weights) != count:
            raise ValueError(f'style_region_weights: {len(weights)} weights for {count} regions')
        if not all(math.isfinite(w) and w >= 0 for w in weights) or not any(w > 0 for w in weights):
            raise ValueError('style_region_weights: finite non-negative numbers with at least one positive')
    return regions, image_regions, weights


def _sized_mask(entry, width, height):
    """A resolved mask at ``width`` x ``height``: bilinear, as fp32 in [0, 1] ([height, width] tensor)."""
    image, divisor = entry
    values = np.asarray(image.resize((width, height), Image.BILINEAR), dtype=np.float32)
    # (an 'F' image's bilinear weights are floats: a value can leave [0, 1] by a rounding, which the plan would refuse)
    values = values / np.float32(divisor) if divisor != 1.0 else values.clip(0, 1)
    return torch.from_numpy(np.ascontiguousarray(values))


def _resolve_weights(weights):
    if isinstance(weights, (list, tuple)):
        return list(weights)
    if isinstance(weights, str) and weights.startswith('synthetic'):
        seed = int(weights.split(':')[1]) if ':' in weights else 0
        return vgg.synthetic_vgg19_weights(seed)
    candidates = []
    if isinstance(weights, str):
        candidates.append(weights)
    if os.environ.get('STYLE_TRANSFER_VGG19'):
        candidates.append(os.environ['STYLE_TRANSFER_VGG19'])
    candidates.append(os.path.expanduser('~/.cache/torch/hub/checkpoints/vgg19-dcbb9e9d.pth'))
    for path in candidates:
        if os.path.exists(path):
            return vgg.load_weights(path)
    raise FileNotFoundError(
        'VGG-19 weights not found. Pass weights=<path to torchvision vgg19-dcbb9e9d.pth>, set '
        "STYLE_TRANSFER_VGG19, or use weights='synthetic' (seeded random weights, tests/benchmarks only).")


class VGGTrunkFunction(torch.autograd.Function):
    """The HIP trunk as a node of an autograd graph: ``taps = VGGTrunkFunction.apply(input, plan, layers, device)``.

    What ``loss.backward()`` of the reference's closure (:472-476) runs through ``VGGFeatures.forward`` (:78-90): the forward
    is ``plan.forward`` and copies of the taps, the backward ``plan.backward`` on the gradients that autograd delivers at the
    taps (st_plan_backward; Normalize and conv1_1's replicate padding included).  Batch 1, first order only.

    A plan holds ONE forward's activations.  The node records ``plan.forward_count``; when another pass has run on the plan
    between this forward and its backward (the style image at the same size, a fused closure), the backward first runs the
    forward again from the saved input - one extra forward pass, same result.  The node keeps the plan alive, so the plan
    cache of VGGFeatures may evict or drop it meanwhile.

    ``plan`` is duck-typed: ``forward(x, last_layer)``, ``feature(layer)``, ``backward(layers, grads)`` and
    ``forward_count``."""

    @staticmethod
    def forward(ctx, input, plan, layers, device):
        if input.shape[0] != 1:
            raise ValueError(f'the HIP trunk takes batch 1, got a batch of {input.shape[0]}')
        layers = tuple(layers)
        plan.forward(input.detach().to(device, torch.float32).contiguous(), max(layers))
        ctx.plan, ctx.layers, ctx.device, ctx.count = plan, layers, device, plan.forward_count
        ctx.save_for_backward(input)
        ctx.set_materialize_grads(False)         # a tap the loss does not use arrives as None and is not seeded
        return tuple(plan.feature(layer) for layer in layers)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_taps):
        (input,) = ctx.saved_tensors
        plan = ctx.plan
        seeded = [(layer, g.detach().to(ctx.device, torch.float32).contiguous())
                  for layer, g in zip(ctx.layers, grad_taps) if g is not None]
        if not seeded:
            return None, None, None, None
        if plan.forward_count != ctx.count:      # the plan's activations are another pass's by now
            plan.forward(input.detach().to(ctx.device, torch.float32).contiguous(), max(ctx.layers))
            ctx.count = plan.forward_count
        grad = plan.backward([layer for layer, _ in seeded], [g for _, g in seeded])
        return grad.reshape(input.shape).to(input.device, input.dtype), None, None, None


class VGGFeatures:
    """Feature extractor facade (reference :20-90) over the HIP trunk; keeps one plan per input size.

    Called under ``torch.enable_grad()`` on an input that requires grad, the taps carry a ``grad_fn`` (VGGTrunkFunction) and
    ``loss.backward()`` reaches the pixels through the HIP trunk, as in the reference's closure; ``feats['input']`` is the
    caller's tensor itself, so a TV term flows through plain autograd.  Otherwise the taps are plain copies."""

    def __init__(self, layers, pooling='max', weights=None, device='cuda:0', precision='fp16x3'):
        if pooling not in vgg.POOLINGS:
            raise KeyError(pooling)
        self.layers = sorted(set(layers))
        self.pooling = pooling
        self.device = torch.device(device)
        self.net = _hip.Net(_resolve_weights(weights), pooling, self.device, precision)
        self._plans = {}

    def plan_for(self, height, width):
        key = (int(height), int(width))
        if key not in self._plans:
            if len(self._plans) >= 4:          # style images of a few sizes; keep the cache small
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = _hip.Plan(self.net, *key)
        return self._plans[key]

    def drop_plans(self):
        self._plans.clear()

    def __call__(self, input, layers=None):
        layers = self.layers if layers is None else sorted(set(layers))
        h, w = input.shape[2:4]
        min_size = vgg.min_size_for(layers)
        if min(h, w) < min_size:
            raise ValueError(f'Input is {h}x{w} but must be at least {min_size}x{min_size}')
        plan = self.plan_for(h, w)
        feats = {'input': input}
        if torch.is_grad_enabled() and input.requires_grad:
            feats.update(zip(layers, VGGTrunkFunction.apply(input, plan, tuple(layers), self.device)))
            return feats
        x = input.detach().to(self.device, torch.float32).contiguous()
        plan.forward(x, max(layers))
        for layer in layers:
            feats[layer] = plan.feature(layer)
        return feats

    forward = __call__


class _DeviceListJob:
    """Control channel of a device-list stylize() (StyleTransfer(devices=[d0, d1, ...]) in ONE process, reference :326-333).

    Rank 0 is the calling process; every other device has a worker process running the same stylize() on its own strip.
    Callbacks fire on rank 0 only - the workers wait at the same iteration for a command on a gloo side group: 0 = go on,
    1 = rank 0's callback asked for the image (get_image / get_image_tensor gather the strips: a collective), 2 = rank 0 was
    interrupted (gather the averaged iterate once more, then everybody leaves), 3 = rank 0's callback failed (leave at once).
    Without a callback there is no per-iteration traffic at all.

    Ctrl-C (reference cli.py:261-266 keeps the image): the workers ignore SIGINT - a terminal delivers it to the whole
    foreground process group - and rank 0 alone decides: inside the callback KeyboardInterrupt is salvaged directly, anywhere
    else the signal only sets `interrupted`, which the next iteration's rendez-vous turns into the same salvage (advisor
    finding of round 5)."""

    def __init__(self, rank, group, st=None):
        self.rank, self.group, self.st = rank, group, st
        self.in_callback = False
        self.interrupted = False
        self.stopped = False

    def _send(self, value):
        import torch.distributed as dist
        dist.broadcast(torch.tensor([value], dtype=torch.int32), src=0, group=self.group)

    def request_gather(self):
        if not self.in_callback:
            raise RuntimeError('StyleTransfer(devices=[...]): while stylize() runs, get_image() / get_image_tensor() may only '
                               'be called from the callback (the strips live in the worker processes)')
        self._send(1)

    def rank0_callback(self, user_callback):
        def fire(it):
            self.in_callback = True
            clean = False
            try:
                user_callback(it)
                if self.interrupted:                     # SIGINT arrived between two rendez-vous
                    raise KeyboardInterrupt
                clean = True
            except KeyboardInterrupt:
                # cli.py:261-266: Ctrl-C keeps what has been computed.  The workers wait at this iteration's rendez-vous:
                # command 2 = gather the averaged iterate once more, then everybody leaves stylize()
                st = self.st
                if st is not None and st.average is not None:
                    self._send(2)
                    local = st.average.get().detach()
                    if st._strip_rows is not None:
                        local = _gather_rows(local, *st._strip_rows)
                    st.image, st.average, st._strip_rows = local, None, None
                    self.stopped = True
                raise
            finally:
                self.in_callback = False
                if not self.stopped:
                    # 0: go on.  3: the callback raised something else - the workers must not run on into collectives
                    # that rank 0 will never join
                    self._send(0 if clean else 3)
                    self.stopped = not clean
        return fire

    def worker_callback(self, st):
        import torch.distributed as dist

        def fire(_it):
            while True:
                cmd = torch.zeros(1, dtype=torch.int32)
                dist.broadcast(cmd, src=0, group=self.group)
                cmd = int(cmd.item())
                if cmd == 0:
                    return
                if cmd == 3:
                    raise _StopDeviceListJob          # rank 0's callback failed: leave without another collective
                if st._strip_rows is not None:
                    st.get_image_tensor()             # joins rank 0's gather
                if cmd == 2:
                    raise _StopDeviceListJob          # rank 0 was interrupted: leave stylize() with it
        return fire


class _StopDeviceListJob(Exception):
    pass


def _device_list_backend(devices):
    """RCCL when every rank has a GPU of its own; a list that names one device twice (tests, a one-GPU box) runs over gloo -
    RCCL refuses two ranks on one device - which is functional, not fast."""
    return 'nccl' if len({str(d) for d in devices}) == len(devices) else 'gloo'


def _device_list_timeout():
    """Seconds a rendez-vous / a gloo collective of the device-list job may take before it fails (a rank that died early must
    not leave the others waiting for the backend's default of 30 minutes)."""
    import datetime
    return datetime.timedelta(seconds=int(os.environ.get('ST_DEVICE_LIST_TIMEOUT', 300)))


def _device_list_worker(rank, world, port, backend, device, ctor, content_image, style_images, kw, has_callback, failures):
    try:
        import signal
        signal.signal(signal.SIGINT, signal.SIG_IGN)         # rank 0 decides (see _DeviceListJob)
        import torch.distributed as dist
        device = torch.device(device)
        torch.cuda.set_device(device)
        init = dict(init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world, timeout=_device_list_timeout())
        if backend == 'nccl':
            init['device_id'] = device
        dist.init_process_group(backend, **init)
        ctl = dist.new_group(backend='gloo')
        if os.environ.get('ST_DEVICE_LIST_INJECT_FAILURE') == str(rank):     # (tests: a worker that dies after the rendez-vous)
            raise RuntimeError('injected worker failure')
        st = StyleTransfer(devices=[device], **ctor)
        st._job = _DeviceListJob(rank, ctl)
        try:
            st.stylize(content_image, style_images, callback=st._job.worker_callback(st) if has_callback else None, **kw)
            torch.cuda.synchronize(device)
            dist.barrier()
        except _StopDeviceListJob:
            torch.cuda.synchronize(device)
        dist.destroy_process_group()
    except BaseException as exc:                             # noqa: BLE001 - reported to rank 0, which raises
        import traceback
        failures.put((rank, f'{type(exc).__name__}: {exc}\n{traceback.format_exc()}'))
        raise


def _device_list_stylize(st, content_image, style_images, kw, callback):
    """stylize() of a StyleTransfer built with a device list: one process per device, this one is rank 0.

    The reference's two-device form (style_transfer.py:326-333, cli.py:214-223) needs no launcher - neither does this: the
    extra ranks are spawned here, joined afterwards, and the result is what `torchrun --nproc-per-node N` gives for the same
    call (it is the same code: strip plans, halo exchange + Gram reductions over RCCL, shard-aware scale transitions)."""
    import socket
    import torch.distributed as dist
    import torch.multiprocessing as mp
    if dist.is_available() and dist.is_initialized():
        raise RuntimeError('StyleTransfer(devices=[...several...]) starts its own ranks; under torchrun pass this rank\'s device only')
    world = len(st.devices)
    backend = _device_list_backend(st.devices)
    if backend == 'nccl' and torch.cuda.device_count() < world:
        raise RuntimeError(f'{world} devices named, {torch.cuda.device_count()} HIP device(s) visible')
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    ctx = mp.get_context('spawn')
    failures = ctx.SimpleQueue()
    env_keep = {k: os.environ.get(k) for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    for k in env_keep:
        os.environ.pop(k, None)                              # (a stale launcher environment must not reach the workers)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    procs = [ctx.Process(target=_device_list_worker, daemon=True,
                         args=(r, world, port, backend, str(st.devices[r]), st._ctor, content_image, style_images, kw,
                               callback is not None, failures))
             for r in range(1, world)]
    for p in procs:
        p.start()
    device = st.devices[0]
    result, error = None, None
    # Watchdog (advisor finding of round 5): a worker that dies early - bad device, out of memory, import error - would leave
    # rank 0 waiting in the rendez-vous or in a collective.  A thread watches the workers; when one has died it aborts the
    # transports rank 0 may be blocked in (the in-library RCCL communicators, torch's RCCL group; a gloo peer's death closes
    # its sockets, which fails the pending operation by itself), and the worker's traceback is what the caller gets.
    import signal
    import threading
    watch = {'stop': False, 'dead': None}

    def watchdog():
        while not watch['stop']:
            dead = [p for p in procs if p.exitcode not in (None, 0)]
            if dead or not failures.empty():
                watch['dead'] = [p.exitcode for p in dead]
                fabric = getattr(st, '_fabric', None)
                try:
                    if fabric is not None and hasattr(fabric, 'close'):
                        fabric.close(abort=True)
                    if backend == 'nccl' and dist.is_initialized():
                        dist.distributed_c10d._abort_process_group()
                except Exception:                            # noqa: BLE001 - best effort: the timeout still bounds the wait
                    pass
                return
            time.sleep(0.25)
    threading.Thread(target=watchdog, daemon=True).start()
    prev_sigint = None
    try:
        torch.cuda.set_device(device)
        init = dict(init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=world, timeout=_device_list_timeout())
        if backend == 'nccl':
            init['device_id'] = device
        dist.init_process_group(backend, **init)
        st._job = _DeviceListJob(0, dist.new_group(backend='gloo'), st)
        if callback is not None and threading.current_thread() is threading.main_thread():
            job = st._job

            def on_sigint(signum, frame):
                if job.in_callback:
                    raise KeyboardInterrupt                  # inside the user's callback: as without this handler
                job.interrupted = True                       # elsewhere: at the next iteration's rendez-vous
            prev_sigint = signal.signal(signal.SIGINT, on_sigint)
        result = st.stylize(content_image, style_images,
                            callback=st._job.rank0_callback(callback) if callback is not None else None, **kw)
        torch.cuda.synchronize(device)
        dist.barrier()
    except BaseException as exc:                             # noqa: BLE001 - re-raised below, after the workers are dealt with
        error = exc
        if st._strip_rows is not None:
            # not salvaged (the exception did not come out of the callback): get_image() must not try a gather without
            # workers - it returns this rank's rows of the averaged iterate
            warnings.warn('device-list stylize() left early: get_image() holds only the first device\'s rows')
            st.image, st.average, st._strip_rows = st.average.get().detach(), None, None
    finally:
        watch['stop'] = True
        if prev_sigint is not None:
            signal.signal(signal.SIGINT, prev_sigint)
        st._job = None
        for k, v in env_keep.items():
            if v is not None:
                os.environ[k] = v
        try:
            if dist.is_initialized():
                from . import sharding
                sharding.release_head_groups()
                dist.destroy_process_group()
        except Exception:                                    # noqa: BLE001
            pass
        for p in procs:
            p.join(timeout=60 if error is None else 5)
            if p.is_alive():
                p.terminate()
    notes = []
    while not failures.empty():
        notes.append('rank %d: %s' % failures.get())
    bad = [p.exitcode for p in procs if p.exitcode not in (0, None)]
    if (notes or watch['dead']) and not isinstance(error, KeyboardInterrupt):
        # the worker's failure is the cause; what rank 0 raised when its transport was aborted under it is the consequence
        raise RuntimeError('a worker of the device-list stylize() failed: ' + ('; '.join(notes) or f'exit codes {bad}')) from error
    if error is not None:
        raise error
    if bad:
        raise RuntimeError(f'a worker of the device-list stylize() failed: exit codes {bad}')
    return result


class StyleTransfer:
    # what the terms are (read by stylize() next to the layer attributes): 'mse' (ContentLossMSE) or 'scaled_mse' (ContentLoss);
    # 'w2' (StyleLossW2) or 'gram' (StyleLoss on Gram matrices).  A name is every layer of the list; a sequence holds exactly
    # one name per entry of content_layers / style_layers, as the reference builds one module per layer.
    content_loss = 'mse'
    style_loss = 'w2'
    # the eps of those modules: None (each kind's default: 1e-4 for 'w2', 1e-8 for 'gram' and 'scaled_mse'; 'mse' has none), a
    # number for every layer of the list, or a sequence with a number or None per layer
    content_eps = None
    style_eps = None
    # 'w2' layers with both covariances restricted to their diagonals (_hip.Plan.set_w2_diagonal, losses.StyleLossW2Diag; the
    # reference has none): the mean / standard-deviation style loss, two memory-bound launches per layer and no C x C work.
    # False, True (every 'w2' layer) or a sequence with one bool per entry of style_layers.  One device only.
    style_diagonal = False
    # 'w2' layers matched on their exact per-channel marginals (_hip.Plan.set_w2_marginal, losses.StyleLossW2Marginal; the
    # reference has none): per channel the sorted tap against the style's sorted tap - the histogram loss in its exact form,
    # which tells sparse from dense where every second-moment statistic cannot.  A segmented sort per layer and iteration.
    # False, True (every 'w2' layer) or a sequence with one bool per entry of style_layers.  Not together with
    # style_diagonal or a custom style_eps on the same layer, nor with style masks or regions.  One device only.
    style_marginal = False
    # 'w2' layers matched on nearest style vectors (_hip.Plan.set_style_nearest, losses.StyleLossNearest; the reference has
    # none): every pixel's feature vector is pulled towards the closest feature vector of the style images - the MRF /
    # neural-neighbour family of style losses, which copies local structure that moment matching smears.  One fused search per
    # layer and iteration: 2 C N M flop for N pixels against M style vectors, and no N x M matrix.  False, True (every 'w2'
    # layer) or a sequence with one bool per entry of style_layers.  Several style images give the union of their vectors in
    # image order; an image of weight 0 is left out, otherwise style_weights do not enter such a layer.  Not together with
    # style_diagonal, style_marginal or a custom style_eps on the same layer, nor with style masks or regions.  One device only.
    style_nearest = False
    # What the style_nearest layers are matched on: 'l2' (the term above), 'cosine' or 'centered_cosine' - the metrics the
    # family is named after (_hip.Plan.set_nearest_metric).  A ReLU tap's vectors differ in length by an order of magnitude across
    # a picture, and a vector's direction is what carries which texture it is: the term is the mean over pixels of one minus the
    # cosine to the best-matching style vector, 'centered_cosine' after subtracting the mean of the style vectors kept (NNST).
    # One name for every flagged layer, or a sequence with one name per entry of style_layers ('l2' on the layers not flagged).
    style_nearest_metric = 'l2'
    # None, or an int K >= 1: when a style tap has more than K pixels the host keeps the columns floor(t M / K), t = 0 ... K - 1,
    # per image and flagged layer.  This is what makes a shallow layer affordable: the search costs 2 C N M flop per iteration
    # (relu1_1 at 512^2 has N = M = 262144).
    style_nearest_samples = None
    # 'w2' layers matched on sliced projections (_hip.Plan.set_style_sliced, losses.StyleLossSliced; the reference has none):
    # the sliced Wasserstein loss of Heitz et al. - the W2 distance between the projections of the iterate's tap and of the
    # style's feature vectors onto random unit directions, new directions at every optimiser step, so that over the run the whole
    # C-dimensional distribution is matched, not two moments of it or its channel marginals.  False, True (every 'w2' layer) or
    # a sequence with one bool per entry of style_layers.  Several style images blend as their projected quantile functions,
    # by style_weights (per direction the Wasserstein barycentre); an image of weight 0 is left out.  Not together with
    # style_diagonal, style_marginal, style_nearest or a custom style_eps on the same layer, nor with style masks or regions.
    # One device only.
    style_sliced = False
    # None (as many directions as the layer has channels) or a multiple of 64 in [64, 512]: the directions per flagged layer.
    style_sliced_projections = None
    # True: new directions at every evaluation of the closure.  False: the directions of epoch 0 throughout, one fixed
    # objective - what optimizer='lbfgs' needs, whose history assumes one.
    style_sliced_resample = True
    # the seed of the directions: the same seed and the same run give the same bits
    style_sliced_seed = 0
    # None, or an int K >= 1: when a style tap has more than K pixels the host keeps the columns floor(t M / K), t = 0 ... K - 1,
    # per image and flagged layer (the style side is projected and sorted again at every step while resampling is on).
    style_sliced_samples = None
    # Spatial masks for the style statistics (read by stylize() too; the reference has none).  style_mask: which pixels of the
    # OUTPUT take the style - a PIL image (read as 'L' / 255) or a 2-D numpy / torch array in [0, 1], resized bilinearly to
    # every scale; the style heads then take mask-weighted moments of the iterate's taps (_hip.Plan.set_style_mask).
    # style_image_masks: a list with one entry per style image, None or a mask of the same forms, resized to that style image
    # at every scale: which of ITS pixels the style is taken from.  One device only.
    style_mask = None
    style_image_masks = None
    # Several style regions, each with its own style (read by stylize() next to the masks; _hip.Plan.set_style_regions).
    # style_regions: None, or a list of 1 to 4 masks in style_mask's forms, resized bilinearly at every scale: where each
    # region's style goes.  style_image_regions: one region index per style image, required then; a region's target for a
    # layer blends its own images' moments with style_weights[i] over the region's sum (style_image_masks still applies per
    # image).  style_region_weights: None (1 / R each) or one finite non-negative number per region, used as given.  Masks
    # may overlap; a pixel in no region takes no style.  Not together with style_mask; one device only.
    style_regions = None
    style_image_regions = None
    style_region_weights = None
    # Spatial weight maps for the content and TV terms (read by stylize() next to style_mask, in its forms, resized bilinearly at
    # every scale; _hip.Plan.set_content_mask / set_tv_mask).  content_mask: where the output stays close to the content image -
    # every content term weighs (F - T) per pixel with the map at its layer's resolution.  tv_mask: where the output is
    # smoothed - each squared difference of the TV term is weighed by the mean of the map at its two end points.  Independent
    # of each other and of the style masks and regions; one device only.
    content_mask = None
    tv_mask = None
    # A Laplacian loss on average-pooled images (Li et al., "Laplacian-Steered Neural Style Transfer"; read by stylize() next
    # to content_mask; _hip.Plan.set_laplacian): laplacian_weight times, per pool size p of laplacian_pools, the mean squared
    # difference between the 4-neighbour Laplacian of avg_pool2d(image, p) and that of the pooled content image - the
    # content's edges and fine structure survive the style.  0: no term.  One device only.
    laplacian_weight = 0.
    laplacian_pools = (4,)

    def __init__(self, devices=['cuda:0'], pooling='max', weights=None, precision='fp16x3'):
        # reference :310 defaults to ['cpu']; this build has no CPU path, so the default is the first HIP device
        self.devices = [torch.device(device) for device in devices]
        self.image = None
        self.average = None

        self.content_layers = list(CONTENT_LAYERS)
        self.style_layers = list(STYLE_LAYERS)
        style_weights = [256, 64, 16, 4, 1]                       # reference :320-322
        weight_sum = sum(abs(w) for w in style_weights)
        self.style_weights = [w / weight_sum for w in style_weights]

        if not 1 <= len(self.devices) <= 8:
            raise ValueError('Only 1 to 8 devices are supported.')           # reference :331: "Only 1 or 2 devices ..."
        if any(d.type != 'cuda' for d in self.devices):
            raise ValueError('This build runs on MI355X only: pass HIP devices (e.g. devices=["cuda:0"]); '
                             'there is no CPU path.')
        # A device LIST (reference :326-333: VGG-19's layers split over two devices, to fit a 24 GB card) is the one-process
        # form of the strip sharding here: stylize() cuts the image into one row strip per device and runs one worker PROCESS
        # per extra device (the MI355X model: one process per GPU over RCCL - the same code path as a torchrun launch), this
        # process being rank 0.  See _device_list_stylize.  The model below serves the single-device calls and rank 0.
        self._ctor = dict(pooling=pooling, weights=weights, precision=precision)
        self._job = None             # the device-list job while its stylize() runs
        # precision: arithmetic of the 3x3 trunk convolutions - 'fp16x3' (default: scaled fp16 planes, fp32-class
        # accuracy, meets the fp32 parity bar), 'bf16x6' (same accuracy, twice the matrix work), 'fp32' (exact
        # fp32 MFMA) or 'bf16x3' (approximate)
        self.model = VGGFeatures(self.style_layers + self.content_layers, pooling=pooling, weights=weights,
                                 device=self.devices[0], precision=precision)
        self._plan = None
        self._strip_rows = None      # (rows, rank) while a strip-sharded scale is running

    # ---- results (reference :335-347) ----
    def get_image_tensor(self):
        """The averaged iterate, 3 x H x W on the compute device (reference :335-336).  While a strip-sharded scale is
        running (one process per GPU) every rank holds only its rows: the strips are gathered here, which makes the
        call a COLLECTIVE in that situation - callbacks fire on every rank at the same iteration, so a callback that
        calls it on every rank (as the CLI's does) is safe; calling it on one rank only would hang."""
        if self.average is None:                      # stylize() has returned: self.image is the gathered result
            return self.image.detach()[0].clamp(0, 1)
        local = self.average.get().detach()
        if self._strip_rows is not None:
            rows, rank = self._strip_rows
            if self._job is not None and rank == 0:
                self._job.request_gather()            # device-list form: the workers join the gather (see _DeviceListJob)
            local = _gather_rows(local, rows, rank)
        return local[0].clamp(0, 1)

    def get_image(self, image_type='pil'):
        if self.average is not None or self.image is not None:
            image = self.get_image_tensor()
            if image_type.lower() == 'pil':
                return to_pil_image(image)
            elif image_type.lower() == 'np_uint16':
                arr = image.cpu().movedim(0, 2).numpy()
                return np.uint16(np.round(arr * 65535))
            else:
                raise ValueError("image_type must be 'pil' or 'np_uint16'")

    # ---- per-scale targets (reference :425-453) ----
    def _build_targets(self, plan, content, style_images, style_weights, scale, style_scale_fac, style_size,
                       style_mask=None, image_masks=None, regions=None):
        device = self.devices[0]
        # masks (_resolve_style_masks' forms): a style image's is in force on ITS plan only while its moments are taken - that
        # plan can be the iterate's own, and this method runs again after the range guard - and the output's goes on last
        masked = style_mask is not None or any(entry is not None for entry in image_masks or [])
        if masked:
            plan.set_style_mask(None)
        # regions (_resolve_style_regions' triple): cleared while the targets are taken, as the mask is, and set last; image i's
        # moments then go to its region's blend alone, with its weight over the region's sum
        region_of = regions[1] if regions else [0] * len(style_images)
        if regions:
            plan.set_style_regions(None)
            sums = [sum(w for w, r in zip(style_weights, region_of) if r == k) for k in range(len(regions[0]))]
            style_weights = [w / sums[r] for w, r in zip(style_weights, region_of)]
        content_layers, style_layers = list(plan.content_layers), list(plan.style_layers)
        # fp16x3's activation-aware range guard (cold path, st_plan_range_guard): the forward arithmetic is checked on every
        # image BEFORE its features become targets; the closure's gradients are checked in stylize() once the targets exist
        guarded = self.model.net.precision == 'fp16x3'
        if guarded:
            plan.range_guard(content)
        if content_layers:
            plan.forward(content, max(content_layers))
            plan.set_content_target_from_forward()
        blends = [{} for _ in range(len(regions[0]) if regions else 1)]
        marginal, quantiles = plan.w2_marginal, {}      # (flagged layers: never with a mask or regions, _resolve_style_marginal)
        nearest, vectors = plan.style_nearest, {}       # (the same, _resolve_style_nearest)
        sliced, sliced_taps = plan.style_sliced, {}     # (the same, _resolve_style_sliced): layer -> ([taps], [weights])
        for i, image in enumerate(style_images):
            blended = blends[region_of[i]]
            if style_size is None:
                sw, sh = size_to_fit(image.size, round(scale * style_scale_fac))
            else:
                sw, sh = size_to_fit(image.size, style_size)
            style = to_tensor(image.resize((sw, sh), Image.BICUBIC))[None].to(device)
            print(f'Processing style image ({sw}x{sh})...')
            if min(sh, sw) < 16:
                raise ValueError(f'Input is {sh}x{sw} but must be at least 16x16')
            splan = plan if (sh, sw) == (plan.height, plan.width) else self.model.plan_for(sh, sw)
            if guarded:
                splan.range_guard(style)
            if not style_layers:
                continue
            splan.forward(style, max(style_layers))
            image_mask = image_masks[i] if image_masks else None
            if image_mask is not None:
                splan.set_style_mask(_sized_mask(image_mask, sw, sh))
            for idx, layer in enumerate(style_layers):
                if sliced[idx]:
                    # a layer matched on sliced projections: the plan keeps every image's feature vectors, in image order with
                    # the image's weight, and derives the target from them under each epoch's directions
                    if style_weights[i] != 0:
                        tap = splan.feature(layer)[0].flatten(1)
                        columns = _nearest_sample_columns(tap.shape[1], self.style_sliced_samples)
                        if len(columns) < tap.shape[1]:
                            tap = tap[:, torch.tensor(columns, device=tap.device)]
                        taps, weights = sliced_taps.setdefault(layer, ([], []))
                        taps.append(tap.clone())
                        weights.append(float(style_weights[i]))
                    continue
                if nearest[idx]:
                    # a layer matched on nearest vectors: the union of the images' feature vectors in image order, an image
                    # of weight 0 left out; the weights do not enter otherwise
                    if style_weights[i] != 0:
                        tap = splan.feature(layer)[0].flatten(1)
                        columns = _nearest_sample_columns(tap.shape[1], self.style_nearest_samples)
                        if len(columns) < tap.shape[1]:
                            tap = tap[:, torch.tensor(columns, device=tap.device)]
                        vectors.setdefault(layer, []).append(tap)
                    continue
                if marginal[idx]:
                    # a layer matched on its marginals: the style tap's quantile functions at the iterate's pixel count,
                    # blended by the images' weights (in one dimension the Wasserstein barycentre)
                    q = _hip.op_resample_quantiles(splan.quantiles(layer), plan.tap_pixels(layer))
                    q *= style_weights[i]
                    if layer not in quantiles:
                        quantiles[layer] = q
                    else:
                        quantiles[layer].add_(q)
                    continue
                mean, srm = splan.moments(layer)
                mean *= style_weights[i]
                srm *= style_weights[i]
                if layer not in blended:
                    blended[layer] = [mean, srm]
                else:
                    blended[layer][0].add_(mean)
                    blended[layer][1].add_(srm)
            if image_mask is not None:
                splan.set_style_mask(None)
        if regions:
            plan.set_style_regions([_sized_mask(entry, plan.width, plan.height) for entry in regions[0]])
            plan.set_region_weights(regions[2])
        for r, blended in enumerate(blends):
            for idx, layer in enumerate(style_layers):
                if sliced[idx]:
                    if layer not in sliced_taps:
                        raise ValueError('style_sliced: every style image has weight 0; a flagged layer needs at least one '
                                         'style image')
                    plan.set_style_sliced_vectors(idx, *sliced_taps[layer])
                elif nearest[idx]:
                    if layer not in vectors:
                        raise ValueError('style_nearest: every style image has weight 0; a flagged layer needs at least one '
                                         'style vector')
                    plan.set_style_vectors(idx, torch.cat(vectors[layer], dim=1))
                elif marginal[idx]:
                    plan.set_style_quantiles(idx, quantiles[layer])
                elif regions:
                    plan.set_region_style_target(r, idx, *blended[layer])
                else:
                    plan.set_style_target(idx, *blended[layer])
        if style_mask is not None:
            plan.set_style_mask(_sized_mask(style_mask, plan.width, plan.height))

    def _guard_rows(self, rows_image, blended=None, content_weight=None, tv_weight=None):
        """st_plan_range_guard on a block of image rows taken as an image of its own (a whole-image plan of that size).
        With ``blended`` (the scale's style targets) the data gradients of one closure are checked too; the content target is
        the block's own forward.  Returns the (forward, backward) layers this call flagged."""
        device = self.devices[0]
        h, w = rows_image.shape[2:]
        probe = _hip.Plan(self.model.net, h, w)
        if blended is not None:
            probe.forward(rows_image, 22)
            probe.set_content_target_from_forward()
            for idx, layer in enumerate(self.style_layers):
                probe.set_style_target(idx, blended[layer][0].contiguous(), blended[layer][1].contiguous())
            probe.set_loss_weights(content_weight, self.style_weights, tv_weight)
        flagged = probe.range_guard(rows_image)
        del probe
        torch.cuda.synchronize(device)
        return flagged

    def _agree_on_wide_layers(self, fabric):
        """The union over the ranks of the layers the range guard has moved to bf16x6: every rank then computes a layer in the
        same arithmetic (a strip's halo rows come from its neighbour's kernels).  Returns True if this rank gained a layer."""
        net = self.model.net
        fwd, bwd = net.wide_layers()
        flags = torch.tensor(fwd + bwd, dtype=torch.float32, device=self.devices[0])
        fabric.allmax(flags)
        merged = [int(v) for v in flags.tolist()]
        net.mark_wide(merged[:13], merged[13:])
        return merged != fwd + bwd

    @staticmethod
    def _style_rows(plan, rows, sh, sw, world):
        """Strips of a style image's forward pass: the optimised image's own strips when the sizes agree (its plan is reused),
        an even split otherwise (a forward pass has no chain owner to relieve)."""
        from . import sharding
        if (sh, sw) == (plan.global_height, plan.width):
            return rows
        return sharding.strip_rows(sh, world)

    def _build_targets_sharded(self, plan, fabric, content, rows, rank, style_images, style_weights, scale,
                               style_scale_fac, style_size):
        """Per-scale targets when the image is cut into row strips: the content target
        from this rank's strip; every style image is cut into its OWN strips (its size is independent of the
        content's) and its raw moment sums are all-reduced - or, when it is too small to give every rank 16
        rows, evaluated whole on every rank (identical kernels on identical inputs: identical results)."""
        from . import sharding
        device, world = self.devices[0], len(rows)
        b, e = rows[rank]
        guarded = self.model.net.precision == 'fp16x3'
        if guarded:
            # the activation-aware range guard of a sharded scale (st_plan_range_guard works on whole-image plans): every rank
            # checks ITS rows as an image of their own - the same kernels on the same statistics, replicate padding where the
            # strip has neighbours - and the ranks take the union of their verdicts before anything becomes a target
            self._guard_rows(content[:, :, b:e].contiguous().to(device))
            for image in style_images:
                if style_size is None:
                    sw, sh = size_to_fit(image.size, round(scale * style_scale_fac))
                else:
                    sw, sh = size_to_fit(image.size, style_size)
                if min(sh, sw) >= 16 and sh // 16 >= world:
                    sb, se = self._style_rows(plan, rows, sh, sw, world)[rank]
                    style = to_tensor(image.resize((sw, sh), Image.BICUBIC))[None]
                    self._guard_rows(style[:, :, sb:se].contiguous().to(device))
            self._agree_on_wide_layers(fabric)
        plan.forward_begin(content[:, :, b:e].contiguous().to(device), 22)
        sharding.run_phases(plan, fabric)
        plan.set_content_target_from_forward()
        blended = {}
        for i, image in enumerate(style_images):
            if style_size is None:
                sw, sh = size_to_fit(image.size, round(scale * style_scale_fac))
            else:
                sw, sh = size_to_fit(image.size, style_size)
            style = to_tensor(image.resize((sw, sh), Image.BICUBIC))[None]
            if rank == 0:
                print(f'Processing style image ({sw}x{sh})...')
            if min(sh, sw) < 16:
                raise ValueError(f'Input is {sh}x{sw} but must be at least 16x16')
            if sh // 16 >= world:
                sb, se = self._style_rows(plan, rows, sh, sw, world)[rank]
                sp = plan if (sh, sw, sb, se) == (plan.global_height, plan.width, b, e) else \
                    sharding.StripPlan(self.model.net, sh, sw, sb, se)
                sp.forward_begin(style[:, :, sb:se].contiguous().to(device), 29)
                sharding.run_phases(sp, fabric)
            else:
                sp = self.model.plan_for(sh, sw)
                sp.forward(style.to(device), 29)
            for level, layer in enumerate(self.style_layers):
                if isinstance(sp, sharding.StripPlan):
                    sums = sp.moment_sums(layer)
                    fabric.allreduce(sums)
                    c = sums.numel()
                    c = int(round((-1 + (1 + 4 * c) ** 0.5) / 2))             # c*c + c entries
                    npix = float((sh >> level) * (sw >> level))
                    srm, mean = (sums[:c * c] / npix).reshape(c, c), sums[c * c:] / npix
                else:
                    mean, srm = sp.moments(layer)
                mean, srm = mean * style_weights[i], srm * style_weights[i]
                if layer not in blended:
                    blended[layer] = [mean, srm]
                else:
                    blended[layer][0] += mean
                    blended[layer][1] += srm
            if sp is not plan:
                del sp
                self.model.drop_plans()
        for idx, layer in enumerate(self.style_layers):
            plan.set_style_target(idx, blended[layer][0].contiguous(), blended[layer][1].contiguous())
        return blended

    def stylize(self, content_image, style_images, *,
                style_weights=None,
                content_weight: float = 0.015,
                tv_weight: float = 2.,
                optimizer: str = 'adam',
                min_scale: int = 128,
                end_scale: int = 512,
                iterations: int = 500,
                initial_iterations: int = 1000,
                step_size: float = 0.02,
                avg_decay: float = 0.99,
                init: str = 'content',
                style_scale_fac: float = 1.,
                style_size: int = None,
                callback=None):

        # the loss's layers are read NOW, as the reference reads them at every scale (:425-453)
        content_layers, style_layers, layer_weights = _resolve_taps(
            self.content_layers, self.style_layers, self.style_weights,
            world=max(len(self.devices), _dist_info()[1]))
        content_loss, style_loss, content_eps, style_eps = _resolve_layer_losses(
            self.content_loss, self.style_loss, self.content_eps, self.style_eps, len(content_layers), len(style_layers),
            world=max(len(self.devices), _dist_info()[1]))
        style_diagonal = _resolve_style_diagonal(self.style_diagonal, style_loss, world=max(len(self.devices), _dist_info()[1]))
        style_mask, image_masks = _resolve_style_masks(self.style_mask, self.style_image_masks, len(style_images),
                                                       world=max(len(self.devices), _dist_info()[1]))
        regions = _resolve_style_regions(self.style_regions, self.style_image_regions, self.style_region_weights,
                                         len(style_images), style_weights, self.style_mask,
                                         world=max(len(self.devices), _dist_info()[1]))
        style_marginal = _resolve_style_marginal(self.style_marginal, style_loss, style_diagonal, style_eps,
                                                 masked=any(value is not None for value in (self.style_mask, self.style_regions,
                                                                                            self.style_image_masks)),
                                                 world=max(len(self.devices), _dist_info()[1]))
        style_nearest = _resolve_style_nearest(self.style_nearest, style_loss, style_diagonal, style_marginal, style_eps,
                                               masked=any(value is not None for value in (self.style_mask, self.style_regions,
                                                                                          self.style_image_masks)),
                                               world=max(len(self.devices), _dist_info()[1]), samples=self.style_nearest_samples)
        style_nearest_metric = _resolve_style_nearest_metric(self.style_nearest_metric, style_nearest,
                                                             world=max(len(self.devices), _dist_info()[1]))
        style_sliced = _resolve_style_sliced(self.style_sliced, style_loss, style_diagonal, style_marginal, style_nearest, style_eps,
                                             masked=any(value is not None for value in (self.style_mask, self.style_regions,
                                                                                        self.style_image_masks)),
                                             world=max(len(self.devices), _dist_info()[1]),
                                             projections=self.style_sliced_projections, samples=self.style_sliced_samples,
                                             resample=self.style_sliced_resample, seed=self.style_sliced_seed, optimizer=optimizer)
        content_map, tv_map = _resolve_weight_maps(self.content_mask, self.tv_mask,
                                                   world=max(len(self.devices), _dist_info()[1]))
        # (the smallest scale's image bounds the pool sizes; a weight of 0 has no term and no size to check)
        smallest = (None, None) if not self.laplacian_weight else size_to_fit(
            content_image.size, gen_scales(min(min_scale, end_scale), end_scale)[0], scale_up=True)
        laplacian = _resolve_laplacian(self.laplacian_weight, self.laplacian_pools, smallest[1], smallest[0],
                                       world=max(len(self.devices), _dist_info()[1]))
        if len(self.devices) > 1 and self._job is None:
            return _device_list_stylize(self, content_image, style_images, dict(
                style_weights=style_weights, content_weight=content_weight, tv_weight=tv_weight, optimizer=optimizer,
                min_scale=min_scale, end_scale=end_scale, iterations=iterations, initial_iterations=initial_iterations,
                step_size=step_size, avg_decay=avg_decay, init=init, style_scale_fac=style_scale_fac, style_size=style_size),
                callback)
        min_scale = min(min_scale, end_scale)
        content_weights = [content_weight / len(content_layers)] * len(content_layers) if content_layers else []

        if style_weights is None:
            style_weights = [1 / len(style_images)] * len(style_images)
        else:
            weight_sum = sum(abs(w) for w in style_weights)
            style_weights = [weight / weight_sum for weight in style_weights]
        if len(style_images) != len(style_weights):
            raise ValueError('style_images and style_weights must have the same length')
        if optimizer not in ('adam', 'lbfgs'):
            raise ValueError("optimizer must be one of 'adam', 'lbfgs'")

        device = self.devices[0]
        scales = gen_scales(min_scale, end_scale)
        # One process per GPU under torch.distributed: the image, the Adam/EMA state and every feature map are cut
        # into row strips (sharding.py) and STAY cut from scale to scale (sharding.resample_strip moves only the few
        # neighbour rows a strip's resample needs); self.image / self.average hold this rank's strip while a sharded
        # scale runs and the gathered full image once the last scale is done.  get_image_tensor() / get_image()
        # gather on demand (a collective: call them on every rank).
        rank, world = _dist_info()
        if world > 8 and optimizer == 'lbfgs':
            # (the strip step's gather area holds at most 8 records: st_qn_strip_state_bytes)
            raise ValueError("optimizer='lbfgs' runs on at most 8 ranks")
        if world > 1:
            from . import sharding
            import torch.distributed as dist
            # ST_FABRIC_HOST_SYNC=1: the conservative transport (what bench.py falls back to, and what the gloo tests
            # run) - every exchange a host-synchronised step, whole convolution launches behind their halos, every
            # rank running every head's chains on all-reduced moments.  The way out if the stream-ordered RCCL path
            # misbehaves on a system: slower, no cross-stream ordering to get wrong.  INTEGRATION.md section 5.
            conservative = os.environ.get('ST_FABRIC_HOST_SYNC') == '1'
            if conservative:
                _hip.set_option('ST_STRIP_OVERLAP', 0)
                _hip.set_option('ST_STRIP_NS_OWNER', 0)
            fabric = sharding.DistFabric(rank, world, host_sync=True if conservative else None)
            # nccl (= RCCL) backend: the closure's exchanges go through the in-library transport (csrc/st_fabric.hip: RCCL
            # operations issued by the library on its own streams, one call per closure); torch.distributed keeps the cold
            # path.  ST_FABRIC_NATIVE=0: torch.distributed for everything (the descriptor form).
            if not conservative and dist.get_backend() == 'nccl' and os.environ.get('ST_FABRIC_NATIVE') != '0':
                try:
                    fabric = sharding.NativeFabric(rank, world, device, cold=fabric)
                except RuntimeError as exc:     # the pre-flight's verdict is agreed over the ranks: all of them land here
                    warnings.warn(f'{exc}; the exchanges go through torch.distributed instead')

        cw, ch = size_to_fit(content_image.size, scales[0], scale_up=True)
        self.image = _starting_image(init, content_image, style_images, style_weights, ch, cw)
        self.image = self.image.to(device)
        if world > 1:
            torch.cuda.synchronize(device)
            dist.broadcast(self.image, src=0)              # the random inits must agree across ranks

        adam = None
        prev_rows, prev_h = None, None       # row strips / height of the previous scale (None: held whole on every rank)
        # ST_STYLIZE_TIMING=1 (measurement aid): per scale, seconds of setup (resample, plan, targets, range guard) and of the
        # iteration loop, each closed by a device synchronisation; read them from self.timing afterwards
        timing = os.environ.get('ST_STYLIZE_TIMING') == '1'
        self.timing = []
        for scale in scales:
            if timing:
                torch.cuda.synchronize(device)
                t_scale = time.perf_counter()
            cw, ch = size_to_fit(content_image.size, scale, scale_up=True)
            content = to_tensor(content_image.resize((cw, ch), Image.BICUBIC))[None]

            # strips need >= 16 rows per rank; a smaller scale runs whole on every rank (same kernels on the same
            # inputs: every rank holds the same result, no exchange needed)
            sharded = world > 1 and ch // 16 >= world
            rows = sharding.strip_rows(ch, world, cw) if sharded else None
            if sharded:
                # shard-aware scale transition (reference :279-295,420,460-462): every rank resamples only its own
                # rows of the image and of the two Adam moments; the few source rows it needs from its neighbours'
                # strips travel point to point (sharding.resample_strip) - nothing is gathered
                b, e = rows[rank]
                old_h = prev_h if prev_h is not None else self.image.shape[2]

                def strip_of(t, mode):
                    return sharding.resample_strip(t.detach(), prev_rows, rank, world, old_h, rows, (ch, cw), mode,
                                                   host_sync=fabric.host_sync)
                self.image = strip_of(self.image, 'bicubic').clamp(0, 1).contiguous()
                if optimizer == 'adam':
                    if adam is None:
                        adam = AdamState(self.image)
                    else:
                        new = AdamState.__new__(AdamState)
                        new.exp_avg = strip_of(adam.exp_avg, 'bicubic')
                        new.exp_avg_sq = strip_of(adam.exp_avg_sq, 'bilinear').relu_().contiguous()
                        new.step = adam.step
                        adam = new
            else:
                if prev_rows is not None:                   # a smaller scale after a sharded one: whole again
                    self.image = _gather_rows(self.image, prev_rows, rank)
                    if adam is not None:
                        adam.exp_avg = _gather_rows(adam.exp_avg, prev_rows, rank)
                        adam.exp_avg_sq = _gather_rows(adam.exp_avg_sq, prev_rows, rank)
                self.image = interpolate(self.image.detach(), (ch, cw), mode='bicubic').clamp(0, 1).contiguous()
                if optimizer == 'adam':
                    adam = AdamState(self.image) if adam is None else adam.rescaled((ch, cw))
            prev_rows, prev_h = rows, ch
            self.average = EMA(self.image, avg_decay)
            self._strip_rows = (rows, rank) if sharded else None

            if rank == 0:
                print(f'Processing content image ({cw}x{ch})...')
            plan = closure = opt = None                    # free the previous scale's plan BEFORE allocating the next
            self._plan = None
            self.model.drop_plans()
            torch.cuda.empty_cache()
            if sharded:
                plan = self._plan = sharding.StripPlan(self.model.net, ch, cw, b, e).set_rank(rank, world)
                blended = self._build_targets_sharded(plan, fabric, content, rows, rank, style_images, style_weights, scale,
                                                      style_scale_fac, style_size)
                grad = torch.empty_like(self.image)
            else:
                min_size = vgg.min_size_for(content_layers + style_layers)
                if min(ch, cw) < min_size:
                    raise ValueError(f'Input is {ch}x{cw} but must be at least {min_size}x{min_size}')
                plan = self._plan = _hip.Plan(self.model.net, ch, cw)
                if (content_layers, style_layers) != (list(plan.content_layers), list(plan.style_layers)):
                    plan.set_taps(content_layers, style_layers)
                if (tuple(content_loss), tuple(style_loss)) != (plan.content_losses, plan.style_losses):
                    plan.set_layer_loss_kinds(content_loss, style_loss)
                if any(value is not None for value in content_eps + style_eps):
                    plan.set_loss_eps(content_eps, style_eps)
                if any(style_diagonal):
                    plan.set_w2_diagonal(style_diagonal)
                if any(style_marginal):
                    plan.set_w2_marginal(style_marginal)
                if any(style_nearest):
                    plan.set_style_nearest(style_nearest)
                    if any(name != _hip.NEAREST_METRICS[0] for name in style_nearest_metric):
                        plan.set_nearest_metric(style_nearest_metric)
                if any(style_sliced):
                    plan.set_style_sliced(style_sliced)
                    for idx, flag in enumerate(style_sliced):
                        if flag:
                            plan.set_sliced_options(idx, self.style_sliced_projections, bool(self.style_sliced_resample))
                    plan.set_sliced_seed(int(self.style_sliced_seed))
                self._build_targets(plan, content.to(device), style_images, style_weights, scale, style_scale_fac,
                                    style_size, style_mask, image_masks, regions)
                # the content and TV maps at this scale's size, on the iterate's plan only and after the targets (which they
                # leave alone): the range guard below then checks the closure that the iterations run
                if content_map is not None:
                    plan.set_content_mask(_sized_mask(content_map, cw, ch))
                if tv_map is not None:
                    plan.set_tv_mask(_sized_mask(tv_map, cw, ch))
                # ... and the Laplacian term, against this scale's content image
                if laplacian is not None:
                    plan.set_laplacian(content.to(device), laplacian[1], laplacian[0])
            plan.set_loss_weights(content_weights, layer_weights, tv_weight)
            if sharded and self.model.net.precision == 'fp16x3':
                # ... sharded: on this rank's rows of the iterate, against the scale's style targets; the union of the ranks'
                # verdicts; forward layers flagged only now have shaped the targets: build them again
                before = self.model.net.wide_layers()
                self._guard_rows(self.image.detach(), blended, content_weights[0], tv_weight)
                self._agree_on_wide_layers(fabric)
                after = self.model.net.wide_layers()
                if after[0] != before[0]:
                    blended = self._build_targets_sharded(plan, fabric, content, rows, rank, style_images, style_weights,
                                                          scale, style_scale_fac, style_size)
                if rank == 0 and after != before:
                    print(f'fp16x3 range guard: bf16x6 for the forward of convs {[i for i, v in enumerate(after[0]) if v]} '
                          f'and the data gradient of convs {[i for i, v in enumerate(after[1]) if v]} from now on')
            if not sharded and self.model.net.precision == 'fp16x3':
                # ... and on the iterate itself, forward and data gradients (one extra closure per scale).  A forward layer
                # flagged only now has already shaped the targets: build them again in the corrected arithmetic.
                fwd, bwd = plan.range_guard(self.image)
                if any(fwd):
                    self._build_targets(plan, content.to(device), style_images, style_weights, scale, style_scale_fac,
                                        style_size, style_mask, image_masks, regions)
                if any(fwd) or any(bwd):
                    print(f'fp16x3 range guard: bf16x6 for the forward of convs {[i for i, v in enumerate(fwd) if v]} and '
                          f'the data gradient of convs {[i for i, v in enumerate(bwd) if v]} from now on')
            self.model.drop_plans()

            if optimizer != 'adam' and sharded:
                # ... on this rank's strip: the same native step, its inner products completed over the ranks by one
                # all-gather of a 72-double record per rank and summed in rank order on the device (no host decision)
                opt = _hip.LBFGS(self.image, rank, world)
            elif optimizer != 'adam':
                # torch.optim.LBFGS(max_iter=1, history_size=10), a fresh one per scale (reference :464-465), as the
                # library's native step: closure, the quasi-Newton update and the EMA in one call, no host decision
                opt = _hip.LBFGS(self.image)

            actual_its = initial_iterations if scale == scales[0] else iterations
            if timing:
                torch.cuda.synchronize(device)
                t_loop = time.perf_counter()
            for i in range(1, actual_its + 1):
                if optimizer == 'adam' and sharded:
                    adam.step += 1
                    plan.closure_begin(self.image, grad)
                    sharding.run_phases(plan, fabric)
                    plan.apply_update(self.image, grad, adam.exp_avg, adam.exp_avg_sq, self.average.value,
                                      adam.step, step_size, 0.9, 0.99, 1e-8, avg_decay)
                    self.average.advance_accum()
                    loss = plan.losses[7]
                elif optimizer == 'adam':
                    adam.step += 1
                    losses = plan.step(self.image, adam.exp_avg, adam.exp_avg_sq, self.average.value,
                                       adam.step, step_size, 0.9, 0.99, 1e-8, avg_decay)
                    self.average.advance_accum()
                    loss = losses[7]
                elif sharded:
                    losses = opt.step_strip(plan, fabric, self.image, grad, self.average.value, avg_decay)
                    self.average.advance_accum()            # no clamp for L-BFGS (reference :482-483)
                    loss = losses[7]
                else:
                    losses = opt.step(plan, self.image, self.average.value, avg_decay)      # (no clamp either)
                    self.average.advance_accum()
                    loss = losses[7]
                if callback is not None:
                    gpu_ram = torch.cuda.max_memory_allocated(device) + plan.device_bytes()
                    callback(STIterate(w=cw, h=ch, i=i, i_max=actual_its, loss=loss.item(),
                                       time=time.time(), gpu_ram=gpu_ram))

            if timing:
                torch.cuda.synchronize(device)
                self.timing.append({'scale': scale, 'size': (cw, ch), 'iterations': actual_its,
                                    'setup_s': t_loop - t_scale, 'loop_s': time.perf_counter() - t_loop})
            # Initialize each new scale with the previous scale's averaged iterate (reference :496-497)
            with torch.no_grad():
                self.image = self.image.detach()
                self.image.copy_(self.average.get())
                if sharded and scale == scales[-1]:         # the result: the full image on every rank
                    self.image = _gather_rows(self.image, rows, rank)
                    self.average = None                     # get_image() falls back to the gathered image
                    self._strip_rows = None

        if world > 1 and isinstance(fabric, sharding.NativeFabric):
            torch.cuda.synchronize(device)
            fabric.close()                                  # every rank is here: a collective destroy of the communicators
        return self.get_image()

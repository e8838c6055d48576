"""The Adam + clamp + EMA update against float64 on every path that applies it, on a real MI355X.

The update is the last arithmetic of every iteration (adam_clamp_ema_element, csrc/st_common.h; host scalars: adam_scalars,
csrc/st_api.hip).  The stylize-level fixtures cannot pin it: trajectories diverge by sign flips and their bars allow for that.
ONE update from a state the test controls has no such freedom.

Reference: ``ref_update64`` - the operation itself in float64 (not the kernel's order of operations, not the fp32-rounded
scalars of AdamScalars).
Floor: ``torch.optim.Adam`` itself in fp32 on the CPU, one step from the same fp32 state, then clamp_ and the reference's EMA
lines (``torch_update32``); its distance from ref_update64, evaluated live for every case.
Metric, per tensor: max over elements of |x - x64| / scale with scale = max(|m_old|, |g|) for exp_avg, max(v_old, g^2) for
exp_avg_sq (a plain max-abs on the moments sees only the largest gradients) and 1 for image and EMA, which live in [0, 1].
Where the scale is 0 (g = m = v = 0) the exact result is 0 and only 0 passes.
Bar: the HIP result within 4 x that case's floor, per tensor, and finite everywhere.  (An op-by-op fp32 emulation of
adam_clamp_ema_element on the CPU stays within 1.72 x the floor on all four tensors over every case of part A; it is not
bit-identical to CPU torch - 1.5 % of exp_avg_sq and 7 % of image values differ in the last bit - so "bit for bit against
torch" is not a property.  Eps on the wrong side of / bc2_sqrt, step - 1 in the bias corrections or an EMA fed the unclamped
pixel sit > 10^4 x the floor at steps <= 10 and > 10^2 x at step 500 with the default hyper-parameters; at lr 0.002,
(0.8, 0.999), step 500 the step mutant is only ~4 x the image's floor: steps <= 10 carry that detection.)

  A. adam_clamp_ema_kernel on a gradient the test chooses (Plan.apply_update), incl. a size whose 3HW exceeds the launch's
     4096 x 256 threads (a second, partial trip of the grid-stride loop);
  B. the update folded into conv1_1's fold kernel (Plan.step, ST_STEP_TAIL=2) at one size per channel-slice count
     (conv_first_fold_kernel<8 / 4 / 2 / 1, true>): bit-identical across the three tails and to apply_update on the closure's
     gradient, and within the bar of float64.
(The general-taps closure's folded update is held bit for bit to apply_update from a non-zero state at steps 2 and 3 by
tests/test_taps_gpu.py test_step_is_loss_and_grad_plus_update_bit_for_bit; strips: tests/test_sharding_gpu.py.)
"""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 4.0                                 # x the case's own floor
SHIPPED = (0.02, 0.9, 0.99, 1e-8, 0.99)   # (lr, beta1, beta2, eps, EMA decay) of the shipped call
HYPER = [SHIPPED,
         (0.5, 0.9, 0.99, 1e-8, 0.9),
         (0.002, 0.8, 0.999, 1e-8, 0.999),
         (0.02, 0.5, 0.9, 1e-3, 0.0)]     # 1 - beta1 at torch's lerp branch point (the kernel keeps one formula); EMA = a copy
STEPS = [1, 2, 3, 10, 100, 500, 1000, 100000]
SENTINEL, GUARD = -12345.5, 256           # 256 floats on either side keep the views 16-byte aligned


# ---- the reference and the floor --------------------------------------------------------------------------------------------
def ref_update64(g, m, v, p, e, step, lr, beta1, beta2, eps, decay):
    """Adam (bias-corrected, eps outside the corrected root) + clamp to [0, 1] + EMA in float64: (m', v', p', e')."""
    g, m, v, p, e = (t.double() for t in (g, m, v, p, e))
    m1 = m + (1 - beta1) * (g - m)
    v1 = beta2 * v + (1 - beta2) * g * g
    denom = v1.sqrt() / math.sqrt(1 - beta2 ** step) + eps
    p1 = (p - lr / (1 - beta1 ** step) * m1 / denom).clamp(0, 1)
    d = float(np.float32(decay))                       # the EMA's decay is an fp32 buffer
    e1 = d * e + (1 - d) * p1
    return m1, v1, p1, e1


def torch_update32(g, m, v, p, e, step, lr, beta1, beta2, eps, decay):
    """torch.optim.Adam's own fp32 step on the CPU from a seeded optimizer state, image.clamp_(0, 1), EMA.update."""
    param = p.clone().requires_grad_(True)
    param.grad = g.clone()
    opt = torch.optim.Adam([param], lr=lr, betas=(beta1, beta2), eps=eps)
    opt.state[param] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
    opt.step()
    assert float(opt.state[param]['step']) == step
    with torch.no_grad():
        param.clamp_(0, 1)
        d = torch.tensor(decay)
        value = e.clone()
        value *= d
        value += (1 - d) * param
    return opt.state[param]['exp_avg'], opt.state[param]['exp_avg_sq'], param.detach(), value


NAMES = ('exp_avg', 'exp_avg_sq', 'image', 'ema')


def distances(got, want64, g, m0, v0):
    """The metric of the module docstring for (m, v, p, e) against float64: four floats."""
    g, m0, v0 = g.double(), m0.double(), v0.double()
    out = []
    for x, x64, scale in zip(got, want64, (torch.maximum(m0.abs(), g.abs()), torch.maximum(v0, g * g), None, None)):
        d = (x.cpu().double() - x64).abs()
        if scale is None:
            out.append(float(d.max()))
            continue
        scaled = scale > 0
        exact = not bool((d[~scaled] != 0).any())             # (a NaN counts as a difference)
        out.append(float((d[scaled] / scale[scaled]).max()) if exact else math.inf)
    return out


def judge(tag, got, state, step, hyper):
    """Prints the case's floors and HIP / floor ratios; returns the failures of the 4 x floor bar."""
    g, m0, v0, p0, e0 = state
    want64 = ref_update64(g, m0, v0, p0, e0, step, *hyper)
    floors = distances(torch_update32(g, m0, v0, p0, e0, step, *hyper), want64, g, m0, v0)
    errs = distances(got, want64, g, m0, v0)
    ratios = [err / floor if floor > 0 else (0.0 if err == 0 else math.inf) for err, floor in zip(errs, floors)]
    print(f'[parity] update {tag}: floor (torch fp32 vs float64) ' + ' '.join(f'{n} {f:.2e}' for n, f in zip(NAMES, floors)) +
          '; hip-vs-float64 / floor ' + ' '.join(f'{n} {r:.2f}' for n, r in zip(NAMES, ratios)))
    failures = [f'{tag}: {n} is not finite' for n, x in zip(NAMES, got) if not bool(torch.isfinite(x).all())]
    failures += [f'{tag}: {n} {err:.3e} from float64 = {r:.2f} x the floor {floor:.3e} (bar {BAR:.0f} x)'
                 for n, err, floor, r in zip(NAMES, errs, floors, ratios) if not err <= BAR * floor]
    return failures


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def moments_like(g, gen):
    """A non-trivial optimizer state around the gradient `g` (CPU): exp_avg of the order of |g| with every 13th element 30 x
    larger (stale momentum: cancellation in g - m), exp_avg_sq in (0.05 ... 1.05) g^2, EMA uniform in [0, 0.3]."""
    n = g.numel()
    idx = torch.arange(n).view(g.shape)
    m = g.abs() * (0.3 + 1.2 * torch.rand(g.shape, generator=gen)) * (torch.randint(0, 2, g.shape, generator=gen) * 2 - 1)
    m = torch.where(idx % 13 == 0, 30 * m, m)
    v = (0.05 + torch.rand(g.shape, generator=gen)) * g * g
    e = 0.3 * torch.rand(g.shape, generator=gen)
    return m.float().contiguous(), v.float().contiguous(), e.float().contiguous()


@functools.lru_cache(maxsize=None)
def chosen_state(h, w):
    """(g, m, v, image, ema), fp32 [1, 3, h, w] on the CPU, shared by every case of a size and never written to.
    Gradient: magnitudes log-uniform over 1e-7 ... 1e-1 with signs; every 7th element ~1e-9 (sqrt(v) comparable to eps); every
    11th exactly 0 together with m = v = 0 (0 / eps: no move, no NaN).  Image uniform in [0, 1] with a fifth of the pixels
    exactly 0, a fifth exactly 1 and a fifth below 0.01: the clamp acts in both directions."""
    gen = torch.Generator().manual_seed(1000 * h + w)
    shape = (1, 3, h, w)
    idx = torch.arange(3 * h * w).view(shape)
    sign = (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()
    g = sign * torch.pow(10.0, -7 + 6 * torch.rand(shape, generator=gen))
    g = torch.where(idx % 7 == 0, sign * 1e-9 * (0.5 + torch.rand(shape, generator=gen)), g)
    g = torch.where(idx % 11 == 0, torch.zeros(shape), g).float().contiguous()
    m, v, e = moments_like(g, gen)
    kind, u = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    p = torch.where(kind < 0.2, torch.zeros(shape), torch.where(kind < 0.4, torch.ones(shape),
                                                                  torch.where(kind < 0.6, 0.01 * u, u))).float().contiguous()
    zero = idx % 11 == 0
    assert not g[zero].any() and not m[zero].any() and not v[zero].any() and bool((v[~zero] > 0).all())
    return g, m, v, p, e


def guarded(t):
    """A copy of `t` on the device as a view into a larger buffer with GUARD sentinel floats on either side: (buffer, view)."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


class State:
    """Guarded device copies of (m, v, image, ema) of one update."""

    def __init__(self, m, v, p, e):
        self.bufs, self.views = zip(*(guarded(t) for t in (m, v, p, e)))
        self.m, self.v, self.p, self.e = self.views

    def tensors(self):
        return tuple(t.clone() for t in self.views)

    def intact(self):
        return all(guards_intact(b) for b in self.bufs)


_PLANS = {}


def _plan(size, weights):
    """One plan per size for the whole module (fp16x3, the shipped arithmetic), targets from tests/synth.py images as in
    test_hot_path_gpu._build_plan."""
    if size not in _PLANS:
        import synth
        from style_transfer import _hip as hip
        h, w = size
        content, style = synth.smooth_image(81, h, w), synth.smooth_image(82, h, w)
        net = hip.Net(weights, 'max', DEV, 'fp16x3')
        plan = hip.Plan(net, h, w)
        plan.forward(content.to(DEV), 22)
        plan.set_content_target_from_forward()
        plan.forward(style.to(DEV), 29)
        for i, layer in enumerate(O.STYLE_LAYERS):
            plan.set_style_target(i, *plan.moments(layer))
        plan.set_loss_weights(0.015, O.STYLE_LAYER_WEIGHTS, 2.0)
        _PLANS[size] = (net, plan)
    return _PLANS[size][1]


# ---- A. the stand-alone kernel ----------------------------------------------------------------------------------------------
# 40 x 48 and 135 x 181 (3HW no multiple of 256, W no multiple of 4): the full grid.  510 x 1022: 3HW = 1.56 M elements exceed
# the launch's 4096 x 256 threads, the grid-stride loop takes a second, partial trip.
CASES_A = [(size, hyper, step) for size in ((40, 48), (135, 181)) for hyper in HYPER for step in STEPS] + \
          [((510, 1022), SHIPPED, step) for step in (1, 10, 1000)]


def _case_id(v):
    if isinstance(v, tuple):
        return 'x'.join(str(x) for x in v) if len(v) == 2 else 'lr{}-b{}-{}-eps{}-d{}'.format(*v)
    return f'step{v}'


@pytest.mark.parametrize('size,hyper,step', CASES_A, ids=_case_id)
def test_update_kernel_on_a_chosen_gradient(size, hyper, step, vgg_weights):
    h, w = size
    assert (3 * h * w > 4096 * 256) == (size == (510, 1022))
    plan = _plan(size, vgg_weights)
    g, m0, v0, p0, e0 = chosen_state(h, w)
    grad = g.to(DEV)
    st = State(m0, v0, p0, e0)
    plan.apply_update(st.p, grad, st.m, st.v, st.e, step, *hyper)
    torch.cuda.synchronize()
    assert torch.equal(grad.cpu(), g), 'the update wrote to its gradient'
    assert st.intact(), 'the update wrote outside a state tensor'
    failures = judge(f'A {h}x{w} step {step} (lr, b1, b2, eps, decay) {hyper}', st.tensors(), (g, m0, v0, p0, e0), step, hyper)
    zero = (g == 0).to(DEV)
    assert not st.m[zero].any() and not st.v[zero].any() and torch.equal(st.p[zero], p0.to(DEV)[zero]), '0 / eps moved a pixel'
    assert not failures, '; '.join(failures)


# ---- B. the update folded into conv1_1's fold kernel ------------------------------------------------------------------------
FOLD_SIZES = {(40, 48): 8, (362, 362): 4, (512, 512): 2, (510, 1022): 1}      # size -> channel slices of conv1_1's dgrad


def _fold_slices(h, w):
    """conv_first_dgrad_parts (csrc/st_conv_first.hip) with the tile constants read from the source, so that a retuning of
    either cannot silently drop an instantiation from the cases."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'style-transfer-pytorch_amd', 'csrc',
                            'st_conv_first.hip')).read()
    ftx, fty = map(int, re.search(r'constexpr int FTX = (\d+), FTY = (\d+);', src).groups())
    assert 'while (parts < 8 && tiles * parts < 512) parts *= 2;' in src, 'conv_first_dgrad_parts changed: revisit FOLD_SIZES'
    tiles = -(-(w + 2) // ftx) * -(-(h + 2) // fty)
    parts = 1
    while parts < 8 and tiles * parts < 512:
        parts *= 2
    return parts


@pytest.mark.parametrize('step', [7, 500], ids=_case_id)
@pytest.mark.parametrize('size', list(FOLD_SIZES), ids=_case_id)
def test_update_folded_into_the_first_convolution(size, step, vgg_weights):
    import synth
    from style_transfer import _hip as hip
    h, w = size
    assert _fold_slices(h, w) == FOLD_SIZES[size]
    plan = _plan(size, vgg_weights)
    image = synth.smooth_image(83, h, w)
    losses, grad = plan.loss_and_grad(image.to(DEV))
    losses, grad = losses.clone(), grad.clone()
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all()
    g = grad.cpu()
    m0, v0, e0 = moments_like(g, torch.Generator().manual_seed(1000 * h + w + step))
    lr = SHIPPED[0]

    runs = {}
    for tail in (2, 1, 0):
        st = State(m0, v0, image, e0)
        with hip.options(ST_STEP_TAIL=tail):
            first_losses = plan.step(st.p, st.m, st.v, st.e, step, lr).clone()
            first = st.tensors()
            # a second iteration, so that a real pass consumes the operand bounds the first one cleared (or did not)
            second_losses = plan.step(st.p, st.m, st.v, st.e, step + 1, lr).clone()
            second = st.tensors()
        torch.cuda.synchronize()
        assert st.intact(), f'ST_STEP_TAIL={tail} wrote outside a state tensor'
        runs[tail] = (first_losses, *first, second_losses, *second)
    # 1. / 4. the three tails agree bit for bit, and the eight losses are the closure's
    for tail in (1, 0):
        for k, (a, b) in enumerate(zip(runs[2], runs[tail])):
            assert torch.equal(a, b), (f'ST_STEP_TAIL=2 vs {tail}', k, float((a - b).abs().max()))
    assert torch.equal(runs[2][0], losses), (runs[2][0], losses)
    assert not torch.equal(runs[2][5], runs[2][0]) and not torch.equal(runs[2][8], runs[2][3])
    # 2. the same element function on the same gradient: apply_update == the step's own update
    st = State(m0, v0, image, e0)
    plan.apply_update(st.p, grad, st.m, st.v, st.e, step, lr)
    torch.cuda.synchronize()
    assert st.intact() and torch.equal(grad, g.to(DEV))
    for n, a, b in zip(NAMES, st.tensors(), runs[0][1:5]):
        assert torch.equal(a, b), (f'apply_update vs ST_STEP_TAIL=0: {n}', float((a - b).abs().max()))
    # 3. the folded kernel's result against float64 on that gradient
    failures = judge(f'B {h}x{w} ({FOLD_SIZES[size]} slices) step {step}', runs[2][1:5], (g, m0, v0, image, e0), step, SHIPPED)
    assert not failures, '; '.join(failures)

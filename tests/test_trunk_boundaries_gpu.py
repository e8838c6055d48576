"""The events that order the plan's streams among themselves (tap_ready, head_done, aux_*, tv_done, ...) are recorded
without a system-scope fence (hipEventDisableSystemFence; profiles/trunk_boundaries.md).  ST_EVENT_SYSTEM_FENCE=1 creates a
plan's events in the former flavour.  Nothing but the packets between the kernels differs, so every value must agree bit
for bit - and a consumer on another stream that read its input before the producer's stores were visible would show here as a
closure that differs from its own repeat."""
import pytest
import torch

import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _plan(hip, weights, content, style, size):
    net = hip.Net(weights, 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, size, size)
    plan.forward(content, 22)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(O.STYLE_LAYERS):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, O.STYLE_LAYER_WEIGHTS, 2.0)
    return net, plan


def test_event_flavours_are_bit_identical(vgg_weights):
    """128^2, the shipped arithmetic: closures, a forward-only pass followed by a closure, and six fused iterations under both
    event flavours.  Losses, gradients, iterates, Adam moments and the EMA are compared with torch.equal."""
    from style_transfer import _hip as hip
    size = 128
    gen = torch.Generator().manual_seed(23)
    content = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    style = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    image0 = torch.rand((1, 3, size, size), generator=gen).to(DEV)

    def run(system_fence):
        out = []
        with hip.options(ST_EVENT_SYSTEM_FENCE=system_fence):      # read when the plan creates its events: first closure
            net, plan = _plan(hip, vgg_weights, content, style, size)
            image = image0.clone()
            for _ in range(3):                                      # a closure and its own repeats
                l, g = plan.loss_and_grad(image)
                out.append((l.clone(), g.clone()))
            plan.forward(image, 29)                                 # forward only ...
            out.append((plan.feature(29).clone(),))
            l, g = plan.loss_and_grad(image)                        # ... then the closure
            out.append((l.clone(), g.clone()))
            m, v, ema = torch.zeros_like(image), torch.zeros_like(image), 0.01 * image
            for step in range(1, 7):
                losses = plan.step(image, m, v, ema, step, 0.02)
                out.append((losses.clone(), image.clone(), m.clone(), v.clone(), ema.clone()))
        torch.cuda.synchronize()
        return out

    new, old, again = run(0), run(1), run(0)
    assert len(new) == len(old) == len(again) == 11
    for k in (1, 2, 4):                                             # repeats and the closure behind a forward-only pass
        for t, u in zip(new[0], new[k]):
            assert torch.equal(t, u), (k, float((t - u).abs().max()))
    for other in (old, again):
        for i, (x, y) in enumerate(zip(new, other)):
            for j, (t, u) in enumerate(zip(x, y)):
                assert torch.equal(t, u), (i, j, float((t - u).abs().max()))
    total = float(new[0][0][7])
    assert total > 0 and abs(total - float(new[0][0][:7].sum())) <= 1e-6 * abs(total)
    print(f'[boundaries] 128^2: 5 closures, a forward pass and 6 iterations bit-identical under both event flavours, '
          f'loss {total:.6f}')

#!/usr/bin/env python3
"""A/B of one optimizer='lbfgs' iteration, in one process: the library's native step (st_plan_lbfgs_step: closure + three
launches, no host decision) against torch.optim.LBFGS(max_iter=1, history_size=10) over plan.loss_and_grad + EMA.update, as
stylize() ran the mode before.  Both arms include the loss.item() a callback does.  The arms alternate, every arm is warmed
up past a full history and timed over at least `--seconds` of work closed by a device synchronise.

    python tools/lbfgs_ab.py [--sizes 128 512 1024] [--repeats 3] [--seconds 1.0] [--trace SIZE]

--trace SIZE: no timing - 12 warm-up and 5 more native iterations at one size, for `rocprofv3 --kernel-trace --stats`
(the step adds lbfgs_dots_kernel, lbfgs_solve_kernel, lbfgs_move_kernel to the closure's launches and copies nothing to
the host)."""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'style-transfer-pytorch_amd'))
sys.path.insert(0, os.path.join(R, 'tests'))
import torch
import synth
from style_transfer import _hip, vgg
from style_transfer.style_transfer import EMA

DEV = 'cuda:0'
WARMUP = 12


def make_plan(net, size):
    plan = _hip.Plan(net, size, size)
    content = synth.smooth_image(21, size, size).to(DEV)
    plan.forward(content, 22)
    plan.set_content_target_from_forward()
    plan.forward(synth.smooth_image(22, size, size).to(DEV), 29)
    for i, layer in enumerate([1, 6, 11, 20, 29]):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [256.0, 64.0, 16.0, 4.0, 1.0], 2.0)
    return plan, content


class TorchArm:
    def __init__(self, plan, content):
        self.plan = plan
        self.image = content.clone().requires_grad_()
        self.average = EMA(self.image, 0.99)
        self.opt = torch.optim.LBFGS([self.image], max_iter=1, history_size=10)

    def closure(self):
        with torch.no_grad():
            losses, grad = self.plan.loss_and_grad(self.image.detach())
        self.image.grad = grad
        return losses[7].clone()

    def iterate(self):
        loss = self.opt.step(self.closure)
        self.average.update(self.image)
        return loss.item()


class NativeArm:
    def __init__(self, plan, content):
        self.plan = plan
        self.image = content.clone()
        self.average = EMA(self.image, 0.99)
        self.opt = _hip.LBFGS(self.image)

    def iterate(self, item=True):
        losses = self.opt.step(self.plan, self.image, self.average.value, 0.99)
        self.average.advance_accum()
        return losses[7].item() if item else None


def timed(arm, seconds):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        arm.iterate()
        n += 1
        if n % 8 == 0 and time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 512, 1024])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--trace', type=int, default=0)
    a = ap.parse_args()
    net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
    if a.trace:
        plan, content = make_plan(net, a.trace)
        arm = NativeArm(plan, content)
        for _ in range(WARMUP + 5):
            arm.iterate(item=False)
        torch.cuda.synchronize()
        print(f'traced {WARMUP + 5} native iterations at {a.trace}^2: {arm.opt.info()}')
        return
    for size in a.sizes:
        plan, content = make_plan(net, size)
        arms = {'torch': TorchArm(plan, content), 'native': NativeArm(plan, content)}
        for arm in arms.values():
            for _ in range(WARMUP):
                arm.iterate()
        rates = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, arm in arms.items():
                rates[k].append(timed(arm, a.seconds))
        t, n = rates['torch'], rates['native']
        verdict = 'native faster in every repeat' if min(n) > max(t) else 'NOT faster in every repeat'
        print(f'{size}^2: torch.optim.LBFGS {" ".join(f"{v:.1f}" for v in t)} it/s (spread {(max(t) - min(t)) / min(t):.1%}); '
              f'native {" ".join(f"{v:.1f}" for v in n)} it/s (spread {(max(n) - min(n)) / min(n):.1%}); '
              f'slowest native / fastest torch = {min(n) / max(t):.3f}: {verdict}', flush=True)
        del arms, plan
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""A/B of one optimizer='lbfgs' iteration ON A STRIP, in one process on one rank over the in-library RCCL transport with
forced collectives: the native strip step (st_plan_qn_strip_step: closure, dots, one ncclAllGather of a 72-double record,
solve, move - no host decision) against sharding.StripLBFGS (torch's recursion in Python, every inner product completed by
a collective of its own and read on the host) + EMA.update, as stylize() ran sharded L-BFGS before.  Both arms include the
loss.item() a callback does.  The arms alternate, every arm is warmed up past a full history and timed over at least
`--seconds` of work closed by a device synchronise.

    ST_FABRIC_FORCE_COLLECTIVES=1 python tools/lbfgs_strips_ab.py [--strips 2048x256 512x256] [--repeats 3] [--seconds 1.0]
                                                                  [--trace WxR]

A strip is WIDTHxROWS (2048x256: one rank of 2048^2 on 8).  --trace WxR: no timing - 12 warm-up and 5 more native
iterations of one strip, for `rocprofv3 --kernel-trace --memory-copy-trace --stats` (between two lbfgs_dots_kernel
dispatches lie the closure's launches, the solve and the move; nothing is copied to the host).

What ONE GPU cannot show: the all-gather's latency between real ranks over xGMI (on one rank RCCL makes it the identity),
and StripLBFGS's collectives between real ranks."""
import argparse
import os
import socket
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'style-transfer-pytorch_amd'))
sys.path.insert(0, os.path.join(R, 'tests'))
import torch
import torch.distributed as dist
import synth
from style_transfer import _hip, sharding, vgg
from style_transfer.style_transfer import EMA

WARMUP = 12


def make_plan(net, fabric, width, rows, dev):
    plan = sharding.StripPlan(net, rows, width, 0, rows).set_rank(0, 1)        # one strip: every row of a rows x width image
    content = synth.smooth_image(21, rows, width).to(dev)
    style = synth.smooth_image(22, rows, width).to(dev)
    sharding.set_targets(plan, content, [style], [1.0], lambda p: sharding.run_phases(p, fabric), fabric.allreduce)
    plan.set_loss_weights(0.015, [256.0, 64.0, 16.0, 4.0, 1.0], 2.0)
    return plan, content


class PythonArm:
    """The sharded L-BFGS branch of stylize() before the native strip step."""

    def __init__(self, plan, fabric, content):
        self.plan, self.fabric = plan, fabric
        self.image = content.clone()
        self.grad = torch.empty_like(self.image)
        self.average = EMA(self.image, 0.99)
        self.opt = sharding.StripLBFGS(self.image, self.grad, fabric.allreduce, fabric.allmax, history_size=10)

    def closure(self):
        self.plan.closure_begin(self.image, self.grad)
        sharding.run_phases(self.plan, self.fabric)
        return self.plan.losses[7].clone()

    def iterate(self):
        loss = self.opt.step(self.closure)
        self.average.update(self.image)
        return loss.item()


class NativeArm:
    def __init__(self, plan, fabric, content):
        self.plan, self.fabric = plan, fabric
        self.image = content.clone()
        self.grad = torch.empty_like(self.image)
        self.average = EMA(self.image, 0.99)
        self.opt = _hip.LBFGS(self.image, 0, 1)

    def iterate(self, item=True):
        losses = self.opt.step_strip(self.plan, self.fabric, self.image, self.grad, self.average.value, 0.99)
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


def strip(text):
    w, r = text.lower().split('x')
    return int(w), int(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--strips', type=strip, nargs='+', default=[(2048, 256), (512, 256)])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--trace', type=strip, default=None)
    a = ap.parse_args()
    if os.environ.get('ST_FABRIC_FORCE_COLLECTIVES') != '1':
        raise SystemExit('run with ST_FABRIC_FORCE_COLLECTIVES=1: on one rank the StripLBFGS arm otherwise issues no collective')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1, device_id=dev)
    fabric = sharding.NativeFabric(0, 1, dev, cold=sharding.DistFabric(0, 1))
    net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', dev, 'fp16x3')
    if a.trace:
        plan, content = make_plan(net, fabric, *a.trace, dev)
        arm = NativeArm(plan, fabric, content)
        for _ in range(WARMUP + 5):
            arm.iterate(item=False)
        torch.cuda.synchronize()
        print(f'traced {WARMUP + 5} native strip iterations at {a.trace[0]}x{a.trace[1]}: {arm.opt.info()}')
    else:
        for width, rows in a.strips:
            plan, content = make_plan(net, fabric, width, rows, dev)
            arms = {'python': PythonArm(plan, fabric, content), 'native': NativeArm(plan, fabric, content)}
            for arm in arms.values():
                for _ in range(WARMUP):
                    arm.iterate()
            rates = {k: [] for k in arms}
            for _ in range(a.repeats):
                for k, arm in arms.items():
                    rates[k].append(timed(arm, a.seconds))
            t, n = rates['python'], rates['native']
            verdict = 'native faster in every repeat' if min(n) > max(t) else 'NOT faster in every repeat'
            print(f'{width}x{rows}: StripLBFGS {" ".join(f"{v:.1f}" for v in t)} it/s (spread {(max(t) - min(t)) / min(t):.1%}); '
                  f'native {" ".join(f"{v:.1f}" for v in n)} it/s (spread {(max(n) - min(n)) / min(n):.1%}); '
                  f'slowest native / fastest StripLBFGS = {min(n) / max(t):.3f}: {verdict}; python arm history '
                  f'{len(arms["python"].opt.old_dirs)}, native {arms["native"].opt.info()}', flush=True)
            del arms, plan
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    fabric.close()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

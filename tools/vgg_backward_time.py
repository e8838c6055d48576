#!/usr/bin/env python3
"""Context for profiles/vgg_backward.md, no pass / fail: the time of plan.forward(29) + plan.backward with the default taps
seeded (features 1, 6, 11, 20, 22, 29; the seventh default tap, 'input', is the caller's tensor and never enters the trunk)
next to plan.loss_and_grad on the same plan at 512^2.  5 warm-ups of each, then blocks of 20 repetitions with one device
synchronise around each block, the two alternating three times.  Prints one JSON line; --out FILE also writes it there.

    python tools/vgg_backward_time.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'style-transfer-pytorch_amd'))
import torch
from style_transfer import _hip, vgg

ap = argparse.ArgumentParser()
ap.add_argument('--out')
args = ap.parse_args()
DEV = 'cuda:0'
torch.manual_seed(0)
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
plan = _hip.Plan(net, 512, 512)
gen = torch.Generator().manual_seed(3)
img = torch.rand((1, 3, 512, 512), generator=gen).to(DEV)
other = torch.rand((1, 3, 512, 512), generator=gen).to(DEV)
plan.forward(other, 29)
plan.set_content_target_from_forward()
for i, layer in enumerate([1, 6, 11, 20, 29]):
    plan.set_style_target(i, *plan.moments(layer))
taps = [1, 6, 11, 20, 22, 29]
plan.forward(img, 29)
grads = [torch.randn(plan.feature(t).shape, generator=gen).to(DEV) for t in taps]
out = torch.empty_like(img)


def vjp():
    plan.forward(img, 29)
    plan.backward(taps, grads, out)


def fused():
    plan.loss_and_grad(img, out)


def block(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for fn in (vjp, fused):
    block(fn, 5)
res = {'vjp_ms': [], 'fused_ms': []}
for _ in range(3):
    res['vjp_ms'].append(block(vjp, 20))
    res['fused_ms'].append(block(fused, 20))
res['plan_bytes'] = plan.device_bytes()
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

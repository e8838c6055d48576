#!/usr/bin/env python3
"""Context for profiles/layer_losses.md, no pass / fail: milliseconds per plan.step at 512^2 on the default layers (content [22]
as 'mse', style [1, 6, 11, 20, 29]) for
  fast            five W2 heads on the closure built for them,
  general         the same plan and targets under ST_GENERAL_TAPS=1 (the general closure, which every other leg runs),
  gram            five Gram heads,
  w2,w2,w2,gram,gram   W2 on the shallow heads (n = 64 / 128 / 256), Gram on relu4_1 / relu5_1 (Plan.set_layer_loss_kinds),
  gram,gram,gram,w2,w2 the other way round.
Each: 10 warm-up steps, then 50 steps between two HIP events; the five alternate three times in one process.  Prints one
JSON line; --out FILE also writes it there.

    python tools/layer_losses_ab.py [--out FILE] [--size N]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'style-transfer-pytorch_amd'))
import torch
from style_transfer import _hip, vgg

ap = argparse.ArgumentParser()
ap.add_argument('--out')
ap.add_argument('--size', type=int, default=512)
args = ap.parse_args()
DEV, SIZE = 'cuda:0', args.size
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
gen = torch.Generator().manual_seed(3)
content = torch.rand((1, 3, SIZE, SIZE), generator=gen).to(DEV)
style = torch.rand((1, 3, SIZE, SIZE), generator=gen).to(DEV)
STYLE = [1, 6, 11, 20, 29]


def make(style_losses):
    plan = _hip.Plan(net, SIZE, SIZE)
    if style_losses != ['w2'] * 5:
        plan.set_layer_loss_kinds(['mse'], style_losses)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    return plan


def timed(plan, force=False):
    x = content.clone()
    m, v, e = torch.zeros_like(x), torch.zeros_like(x), 0.01 * x
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with _hip.options(ST_GENERAL_TAPS=1 if force else 0):
        for k in range(1, 11):
            plan.step(x, m, v, e, k, 0.02)
        start.record()
        for k in range(11, 61):
            plan.step(x, m, v, e, k, 0.02)
        stop.record()
        torch.cuda.synchronize()
    return start.elapsed_time(stop) / 50


LEGS = [['gram'] * 5, ['w2', 'w2', 'w2', 'gram', 'gram'], ['gram', 'gram', 'gram', 'w2', 'w2']]
default = make(['w2'] * 5)
plans = {','.join(leg): make(leg) for leg in LEGS}
res = {'size': SIZE, 'fast_ms': [], 'general_ms': []}
res.update({f'{name}_ms': [] for name in plans})
res['device_bytes'] = {'w2,w2,w2,w2,w2': default.device_bytes(), **{name: plan.device_bytes() for name, plan in plans.items()}}
for _ in range(3):
    res['fast_ms'].append(timed(default))
    res['general_ms'].append(timed(default, force=True))
    for name, plan in plans.items():
        res[f'{name}_ms'].append(timed(plan))
for name in plans:
    res[f'{name}_over_general'] = min(res[f'{name}_ms']) / min(res['general_ms'])
    res[f'{name}_over_fast'] = min(res[f'{name}_ms']) / min(res['fast_ms'])
res['general_over_fast'] = min(res['general_ms']) / min(res['fast_ms'])
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

#!/usr/bin/env python3
"""Context for profiles/style_mask.md, no pass / fail: milliseconds per plan.step at 512^2 on the default layers (content [22],
style [1, 6, 11, 20, 29]) for three arms, all on the general closure:
  general         five W2 heads, no mask (ST_GENERAL_TAPS=1: the closure a mask sends the default configuration to),
  masked          the same plan and targets with a style mask (Plan.set_style_mask: masked Gram staging, one pointwise
                  launch per head),
  masked_gram     five Gram heads with the same mask,
and, for scale, `fast`: the default closure, which an unmasked default plan runs.  The mask is a horizontal ramp with a
quarter of exact zeros.  Each: 10 warm-up steps, then 50 steps between two HIP events; the arms alternate three times in one
process.  Prints one JSON line; --out FILE also writes it there.

    python tools/style_mask_ab.py [--out FILE] [--size N]
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
x = torch.arange(SIZE, dtype=torch.float32) / (SIZE - 1)
MASK = (2 * (x - 0.25)).clamp(0, 1)[None, :].repeat(SIZE, 1).contiguous().to(DEV)


def make(style_loss):
    plan = _hip.Plan(net, SIZE, SIZE)
    if style_loss != 'w2':
        plan.set_loss_kinds('mse', style_loss)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    return plan


def timed(plan, mask=None, force=False):
    plan.set_style_mask(mask)
    img = content.clone()
    m, v, e = torch.zeros_like(img), torch.zeros_like(img), 0.01 * img
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with _hip.options(ST_GENERAL_TAPS=1 if force else 0):
        for k in range(1, 11):
            plan.step(img, m, v, e, k, 0.02)
        start.record()
        for k in range(11, 61):
            plan.step(img, m, v, e, k, 0.02)
        stop.record()
        torch.cuda.synchronize()
    plan.set_style_mask(None)
    return start.elapsed_time(stop) / 50


w2, gram = make('w2'), make('gram')
res = {'size': SIZE, 'fast_ms': [], 'general_ms': [], 'masked_ms': [], 'masked_gram_ms': []}
for _ in range(3):
    res['fast_ms'].append(timed(w2))
    res['general_ms'].append(timed(w2, force=True))
    res['masked_ms'].append(timed(w2, MASK))
    res['masked_gram_ms'].append(timed(gram, MASK))
res['masked_over_general'] = min(res['masked_ms']) / min(res['general_ms'])
res['masked_over_fast'] = min(res['masked_ms']) / min(res['fast_ms'])
res['general_over_fast'] = min(res['general_ms']) / min(res['fast_ms'])
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

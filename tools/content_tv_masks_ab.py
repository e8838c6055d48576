#!/usr/bin/env python3
"""Context for profiles/content_tv_masks.md, no pass / fail: milliseconds per plan.step at 512^2 on the default layers (content
[22], style [1, 6, 11, 20, 29]) for four arms, all on the general closure:
  general         no map (ST_GENERAL_TAPS=1: the closure a map sends the default configuration to),
  content         the same plan and targets with a content map (Plan.set_content_mask: the weighted content launch),
  tv              with a TV map (Plan.set_tv_mask: the weighted TV kernels),
  both            with both,
and, for scale, `fast`: the default closure, which a default plan without maps runs.  The map is a horizontal ramp with a
quarter of exact zeros.  Each: 10 warm-up steps, then 50 steps between two HIP events; the arms alternate three times in one
process.  Prints one JSON line; --out FILE also writes it there.

    python tools/content_tv_masks_ab.py [--out FILE] [--size N]
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
MAP = (2 * (x - 0.25)).clamp(0, 1)[None, :].repeat(SIZE, 1).contiguous().to(DEV)

plan = _hip.Plan(net, SIZE, SIZE)
plan.forward(content, 29)
plan.set_content_target_from_forward()
plan.forward(style, 29)
for i, layer in enumerate(STYLE):
    plan.set_style_target(i, *plan.moments(layer))
plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)


def timed(content_map=None, tv_map=None, force=False):
    plan.set_content_mask(content_map)
    plan.set_tv_mask(tv_map)
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
    plan.set_content_mask(None)
    plan.set_tv_mask(None)
    return start.elapsed_time(stop) / 50


res = {'size': SIZE, 'fast_ms': [], 'general_ms': [], 'content_ms': [], 'tv_ms': [], 'both_ms': []}
for _ in range(3):
    res['fast_ms'].append(timed())
    res['general_ms'].append(timed(force=True))
    res['content_ms'].append(timed(content_map=MAP))
    res['tv_ms'].append(timed(tv_map=MAP))
    res['both_ms'].append(timed(content_map=MAP, tv_map=MAP))
for arm in ('content', 'tv', 'both'):
    res[f'{arm}_over_general'] = min(res[f'{arm}_ms']) / min(res['general_ms'])
res['general_over_fast'] = min(res['general_ms']) / min(res['fast_ms'])
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

#!/usr/bin/env python3
"""Context for profiles/style_regions.md, no pass / fail: milliseconds per plan.step at 512^2 on the default layers (content
[22], style [1, 6, 11, 20, 29]) for four arms, all on the general closure, with W2 heads and again with Gram heads:
  masked          a style mask (Plan.set_style_mask): what a plan did before it could take regions,
  regions_1       the same mask as ONE region of weight 1 (Plan.set_style_regions): bit for bit the masked plan's results,
  regions_2       two regions, the mask and its complement, with a style each,
  regions_3       three regions: those two and a binary quadrant.
Region r's targets are the moments of a style image of its own.  Each arm: 10 warm-up steps, then 150 steps between two HIP
events; the arms alternate three times in one process.  Prints one JSON line; --out FILE also writes it there.  The one thing
to read off: whether regions_1 lies within the spread of masked's repeats.

    python tools/style_regions_ab.py [--out FILE] [--size N]
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
styles = [torch.rand((1, 3, SIZE, SIZE), generator=gen).to(DEV) for _ in range(3)]
STYLE = [1, 6, 11, 20, 29]
x = torch.arange(SIZE, dtype=torch.float32) / (SIZE - 1)
RAMP = (2 * (x - 0.25)).clamp(0, 1)[None, :].repeat(SIZE, 1).contiguous().to(DEV)
QUADRANT = torch.zeros((SIZE, SIZE))
QUADRANT[:SIZE // 2, :SIZE // 2] = 1
MASKS = [RAMP, (1 - RAMP).contiguous(), QUADRANT.to(DEV)]


def make(style_loss):
    plan = _hip.Plan(net, SIZE, SIZE)
    if style_loss != 'w2':
        plan.set_loss_kinds('mse', style_loss)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    moments = []
    for style in styles:
        plan.forward(style, 29)
        moments.append([plan.moments(layer) for layer in STYLE])
    for i in range(len(STYLE)):
        plan.set_style_target(i, *moments[0][i])
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    return plan, moments


def timed(made, regions):
    """regions 0: the style mask; R >= 1: that many regions."""
    plan, moments = made
    if regions == 0:
        plan.set_style_mask(RAMP)
    else:
        plan.set_style_regions(MASKS[:regions])
        for r in range(1, regions):
            for i in range(len(STYLE)):
                plan.set_region_style_target(r, i, *moments[r][i])
    img = content.clone()
    m, v, e = torch.zeros_like(img), torch.zeros_like(img), 0.01 * img
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(1, 11):
        plan.step(img, m, v, e, k, 0.02)
    start.record()
    for k in range(11, 161):
        plan.step(img, m, v, e, k, 0.02)
    stop.record()
    torch.cuda.synchronize()
    plan.set_style_mask(None)
    plan.set_style_regions(None)
    return start.elapsed_time(stop) / 150


ARMS = [('masked', 0), ('regions_1', 1), ('regions_2', 2), ('regions_3', 3)]
res = {'size': SIZE}
for kind in ('w2', 'gram'):
    made = make(kind)
    out = res[kind] = {f'{name}_ms': [] for name, _ in ARMS}
    for _ in range(3):
        for name, regions in ARMS:
            out[f'{name}_ms'].append(timed(made, regions))
    lo, hi = min(out['masked_ms']), max(out['masked_ms'])
    out['regions_1_within_masked_spread'] = all(lo <= t <= hi for t in out['regions_1_ms'])
    out['regions_1_over_masked'] = min(out['regions_1_ms']) / lo
    out['ms_per_extra_region'] = (min(out['regions_3_ms']) - min(out['regions_1_ms'])) / 2
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

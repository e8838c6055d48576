#!/usr/bin/env python3
"""Context for profiles/general_taps.md, no pass / fail: milliseconds per plan.step at 512^2 for
  fast      the default layers on the closure built for them,
  general   the same plan and targets under ST_GENERAL_TAPS=1 (the general closure of csrc/st_taps.hip),
  config_b  content [22, 29], style [1, 6, 11, 20, 29] (two content layers, 29 in both lists) on the general closure.
Each: 10 warm-up steps, then 50 steps between two HIP events; the three alternate three times.  Prints one JSON line; --out FILE
also writes it there.

    python tools/general_taps_time.py [--out FILE]
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
args = ap.parse_args()
DEV, SIZE = 'cuda:0', 512
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
gen = torch.Generator().manual_seed(3)
content = torch.rand((1, 3, SIZE, SIZE), generator=gen).to(DEV)
style = torch.rand((1, 3, SIZE, SIZE), generator=gen).to(DEV)
STYLE = [1, 6, 11, 20, 29]


def make(content_layers):
    plan = _hip.Plan(net, SIZE, SIZE)
    if content_layers != [22]:
        plan.set_taps(content_layers, STYLE)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015 / len(content_layers), [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    return plan


def timed(plan, force):
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


default, config_b = make([22]), make([22, 29])
res = {'fast_ms': [], 'general_ms': [], 'config_b_ms': []}
for _ in range(3):
    res['fast_ms'].append(timed(default, False))
    res['general_ms'].append(timed(default, True))
    res['config_b_ms'].append(timed(config_b, False))
res['general_over_fast'] = min(res['general_ms']) / min(res['fast_ms'])
res['config_b_over_fast'] = min(res['config_b_ms']) / min(res['fast_ms'])
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

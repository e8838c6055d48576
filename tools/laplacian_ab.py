#!/usr/bin/env python3
"""Context for profiles/laplacian.md, no pass / fail: milliseconds per plan.step at 512^2 on the default layers (content [22],
style [1, 6, 11, 20, 29]) for four arms, all on the general closure:
  general         no Laplacian (ST_GENERAL_TAPS=1: the closure a Laplacian sends the default configuration to),
  pools_4         the same plan and targets with Plan.set_laplacian(content, (4,)): pool, residual and gradient add,
  pools_1         pools (1,): no pool launch, the residual pass at the image's size,
  pools_4_16      pools (4, 16): six launches,
and, for scale, `fast`: the default closure, which a default plan without a Laplacian runs.  Each: 10 warm-up steps, then 50
steps between two HIP events; the arms alternate three times in one process.  Prints one JSON line; --out FILE also writes it
there.

    python tools/laplacian_ab.py [--out FILE] [--size N]
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
start_image = torch.rand((1, 3, SIZE, SIZE), generator=gen).to(DEV)
STYLE = [1, 6, 11, 20, 29]

plan = _hip.Plan(net, SIZE, SIZE)
plan.forward(content, 29)
plan.set_content_target_from_forward()
plan.forward(style, 29)
for i, layer in enumerate(STYLE):
    plan.set_style_target(i, *plan.moments(layer))
plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)


def timed(pools=None, force=False):
    plan.set_laplacian(None if pools is None else content, pools or (4,), 1.0)
    img = start_image.clone()
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
    plan.set_laplacian(None)
    return start.elapsed_time(stop) / 50


ARMS = {'pools_4': (4,), 'pools_1': (1,), 'pools_4_16': (4, 16)}
res = {'size': SIZE, 'fast_ms': [], 'general_ms': [], **{f'{arm}_ms': [] for arm in ARMS}}
for _ in range(3):
    res['fast_ms'].append(timed())
    res['general_ms'].append(timed(force=True))
    for arm, pools in ARMS.items():
        res[f'{arm}_ms'].append(timed(pools))
for arm in ARMS:
    res[f'{arm}_over_general'] = min(res[f'{arm}_ms']) / min(res['general_ms'])
    res[f'{arm}_minus_general_us'] = 1e3 * (min(res[f'{arm}_ms']) - min(res['general_ms']))
res['general_over_fast'] = min(res['general_ms']) / min(res['fast_ms'])
res['device'] = torch.cuda.get_device_name(0)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))

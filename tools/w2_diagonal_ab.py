#!/usr/bin/env python3
"""Context for profiles/w2_diagonal.md, no pass / fail: milliseconds per plan.step on the default layers (content [22] as 'mse',
style [1, 6, 11, 20, 29]), at 512^2 and at 128^2, for
  fast            five full W2 heads on the closure built for them,
  general         the same plan and targets under ST_GENERAL_TAPS=1 (the general closure, which every other arm runs),
  gram            five Gram heads (Plan.set_layer_loss_kinds),
  w2,w2,w2,gram,gram   the mixed list of profiles/layer_losses.md,
  diagonal        five diagonal W2 heads (Plan.set_w2_diagonal),
  w2,w2,w2,diag,diag   full W2 on the shallow heads (n = 64 / 128 / 256), diagonal on relu4_1 / relu5_1.
Each: 10 warm-up steps, then 50 steps between two HIP events; the arms alternate three times in one process per size.  Prints
one JSON line; --out FILE also writes it there and --markdown FILE writes the table of profiles/w2_diagonal.md (per arm the
best of the three repeats, all three, and their spread (max - min) / min).

    python tools/w2_diagonal_ab.py [--out FILE] [--markdown FILE] [--sizes 512 128]
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
ap.add_argument('--markdown')
ap.add_argument('--sizes', type=int, nargs='+', default=[512, 128])
args = ap.parse_args()
DEV = 'cuda:0'
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
STYLE = [1, 6, 11, 20, 29]
W2 = ['w2'] * 5
ARMS = {                       # name: (style kinds, diagonal flags)
    'gram': (['gram'] * 5, None),
    'w2,w2,w2,gram,gram': (['w2', 'w2', 'w2', 'gram', 'gram'], None),
    'diagonal': (W2, [True] * 5),
    'w2,w2,w2,diag,diag': (W2, [False, False, False, True, True]),
}


def make(size, content, style, kinds, flags):
    plan = _hip.Plan(net, size, size)
    if kinds != W2:
        plan.set_layer_loss_kinds(['mse'], kinds)
    if flags is not None:
        plan.set_w2_diagonal(flags)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    return plan


def timed(plan, content, force=False):
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


res = {'device': torch.cuda.get_device_name(0), 'sizes': {}}
for size in args.sizes:
    gen = torch.Generator().manual_seed(3)
    content = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    style = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    default = make(size, content, style, W2, None)
    plans = {name: make(size, content, style, *arm) for name, arm in ARMS.items()}
    ms = {name: [] for name in ['fast', 'general', *plans]}
    for _ in range(3):
        ms['fast'].append(timed(default, content))
        ms['general'].append(timed(default, content, force=True))
        for name, plan in plans.items():
            ms[name].append(timed(plan, content))
    res['sizes'][str(size)] = {
        'ms': ms,
        'device_bytes': {'fast': default.device_bytes(), **{name: plan.device_bytes() for name, plan in plans.items()}},
        'diagonal_over_gram': min(ms['diagonal']) / min(ms['gram']),
        'deep_diagonal_over_deep_gram': min(ms['w2,w2,w2,diag,diag']) / min(ms['w2,w2,w2,gram,gram']),
    }
    del default, plans
    torch.cuda.empty_cache()

if args.out:
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
if args.markdown:
    with open(args.markdown, 'w') as f:
        for size, entry in res['sizes'].items():
            f.write(f'{size} x {size}, ms per `plan.step` ({res["device"]}):\n\n')
            f.write('| arm | best | three repeats | spread |\n|---|---|---|---|\n')
            for name, values in entry['ms'].items():
                f.write(f'| `{name}` | {min(values):.3f} | {", ".join(f"{v:.3f}" for v in values)} | '
                        f'{(max(values) - min(values)) / min(values) * 100:.1f} % |\n')
            f.write('\n')
print(json.dumps(res))

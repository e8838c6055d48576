#!/usr/bin/env python3
"""Context for profiles/style_sliced.md, no pass / fail: milliseconds per plan.step on the default layers (content [22] as 'mse',
style [1, 6, 11, 20, 29]), at 128^2 and at 512^2, for
  fast                    five full W2 heads on the closure built for them,
  marginal                five marginal heads (Plan.set_w2_marginal),
  sliced                  five sliced heads (Plan.set_style_sliced), P = C, new directions at every step,
  sliced-fixed            the same with resampling off: the directions and the target of epoch 0 throughout,
  w2,w2,w2,sliced,sliced  full W2 on the shallow heads, sliced on relu4_1 / relu5_1, resampling on,
  sliced-16384            five sliced heads, each style tap cut to at most 16384 evenly spaced vectors (style_sliced_samples).
Each: 10 warm-up steps, then 50 steps between two HIP events; the arms alternate three times in one process per size.  Then the
pieces of ONE relu1_1 head through the standalone operators on the plan's own taps, 20 calls between two events each: the direction
kernel, one projection (st_op_conv1x1, fp16x3, bounds measured inside), one sort of P rows (st_op_channel_sort), one resample, the
style side as a whole (st_op_sliced_target: project, sort, unpack, resample, blend) and the tap side as a whole (st_op_sliced_loss:
project, sort, residual, bound of G, back-project).  Prints one JSON line; --out FILE also writes it there and --markdown FILE
writes the tables of profiles/style_sliced.md.

    python tools/style_sliced_ab.py [--out FILE] [--markdown FILE] [--sizes 128 512]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'style-transfer-pytorch_amd'))
import torch
from style_transfer import _hip, vgg
from style_transfer.style_transfer import _nearest_sample_columns

ap = argparse.ArgumentParser()
ap.add_argument('--out')
ap.add_argument('--markdown')
ap.add_argument('--sizes', type=int, nargs='+', default=[128, 512])
args = ap.parse_args()
DEV = 'cuda:0'
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
STYLE = [1, 6, 11, 20, 29]
ALL = [True] * 5
DEEP = [False, False, False, True, True]
ARMS = {                       # name: (marginal flags, sliced flags, resample, samples)
    'marginal': (ALL, None, True, None),
    'sliced': (None, ALL, True, None),
    'sliced-fixed': (None, ALL, False, None),
    'w2,w2,w2,sliced,sliced': (None, DEEP, True, None),
    'sliced-16384': (None, ALL, True, 16384),
}


def make(size, content, style, marg, sliced, resample, samples):
    plan = _hip.Plan(net, size, size)
    if marg is not None:
        plan.set_w2_marginal(marg)
    if sliced is not None:
        plan.set_style_sliced(sliced)
        for i, flag in enumerate(sliced):
            if flag:
                plan.set_sliced_options(i, None, resample)
        plan.set_sliced_seed(1)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        if sliced is not None and sliced[i]:
            tap = plan.feature(layer)[0].flatten(1)
            columns = _nearest_sample_columns(tap.shape[1], samples)
            plan.set_style_sliced_vectors(i, tap if len(columns) == tap.shape[1] else tap[:, torch.tensor(columns, device=DEV)])
        elif marg is not None and marg[i]:
            plan.set_style_quantiles(i, plan.quantiles(layer))
        else:
            plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    return plan


def events(fn, warm, count):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warm):
        fn(k)
    start.record()
    for k in range(warm, warm + count):
        fn(k)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / count


def timed(plan, content):
    x = content.clone()
    m, v, e = torch.zeros_like(x), torch.zeros_like(x), 0.01 * x
    return events(lambda k: plan.step(x, m, v, e, k + 1, 0.02), 10, 50)


res = {'device': torch.cuda.get_device_name(0), 'sizes': {}}
for size in args.sizes:
    gen = torch.Generator().manual_seed(3)
    content = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    style = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    default = make(size, content, style, None, None, True, None)
    plans = {name: make(size, content, style, *arm) for name, arm in ARMS.items()}
    ms = {name: [] for name in ['fast', *plans]}
    for _ in range(3):
        ms['fast'].append(timed(default, content))
        for name, plan in plans.items():
            ms[name].append(timed(plan, content))
    # the pieces of one relu1_1 head: the iterate's tap against the style's, C = P = 64
    default.forward(style, 29)
    vectors = default.feature(1)[0].flatten(1).contiguous()
    default.forward(content, 29)
    feat = default.feature(1)[0].flatten(1).contiguous()
    c, n = int(feat.shape[0]), int(feat.shape[1])
    r, rt = _hip.op_sliced_directions(1, 0, 0, c, c, DEV)
    target = _hip.op_sliced_target(vectors, r, rt, n)
    y = _hip.op_conv1x1(feat, r, None, 4)
    pieces = {
        'directions': events(lambda k: _hip.op_sliced_directions(1, 0, k, c, c, DEV), 3, 20),
        'one projection (with its two bound passes)': events(lambda k: _hip.op_conv1x1(feat, r, None, 4), 3, 20),
        'one sort of P rows': events(lambda k: _hip.op_channel_sort(y, values=False, indices=False), 3, 20),
        'one resample': events(lambda k: _hip.op_resample_quantiles(y, n + 1), 3, 20),
        'style side (project, sort, unpack, blend)': events(lambda k: _hip.op_sliced_target(vectors, r, rt, n), 3, 20),
        'tap side (project, sort, residual, bound, back-project)': events(lambda k: _hip.op_sliced_loss(feat, r, rt, target), 3, 20),
        'marginal head (sort, residual)': events(lambda k: _hip.op_w2_marginal_loss(feat, target), 3, 20),
    }
    res['sizes'][str(size)] = {
        'ms': ms,
        'relu1_1': {'shape': [c, c, n], 'ms': pieces},
        'device_bytes': {'fast': default.device_bytes(), **{name: plan.device_bytes() for name, plan in plans.items()}},
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
            head = entry['relu1_1']
            f.write(f'\n{size} x {size}, the pieces of one relu1_1 head, C x P x N = {head["shape"][0]} x {head["shape"][1]} x {head["shape"][2]}, '
                    'ms per call of the standalone operator:\n\n| piece | ms |\n|---|---|\n')
            for name, value in head['ms'].items():
                f.write(f'| {name} | {value:.3f} |\n')
            f.write('\n')
print(json.dumps(res))

#!/usr/bin/env python3
"""Context for profiles/nearest_cosine.md, no pass / fail: milliseconds per plan.step on the default layers (content [22] as 'mse',
style [1, 6, 11, 20, 29]), at 128^2 and at 512^2, for the arms of profiles/style_nearest.md under two metrics:
  w2,w2,w2,near,near   full W2 on the shallow heads, nearest on relu4_1 / relu5_1 against every style vector,
  nearest-4096         five nearest heads, each against at most 4096 evenly spaced style vectors,
each with the L2 metric and with 'centered_cosine' (Plan.set_nearest_metric), so that the extra cost of the cosine finish pass over
the L2 one is the difference of two measured rows.  Each: 10 warm-up steps, then 50 steps between two HIP events; the arms
alternate three times in one process per size.  Then the whole head alone at relu4_1 (st_op_nearest_loss against
st_op_nearest_cosine_loss) and the search alone, 20 calls between two events.  Prints one JSON line; --out FILE also writes it
there and --markdown FILE writes the tables of profiles/nearest_cosine.md.

    python tools/nearest_cosine_ab.py [--out FILE] [--markdown FILE] [--sizes 128 512]
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
DEEP = [False, False, False, True, True]
ARMS = {                       # name: (nearest flags, samples, metric)
    'w2,w2,w2,near,near l2': (DEEP, None, 'l2'),
    'w2,w2,w2,near,near centered_cosine': (DEEP, None, 'centered_cosine'),
    'nearest-4096 l2': ([True] * 5, 4096, 'l2'),
    'nearest-4096 centered_cosine': ([True] * 5, 4096, 'centered_cosine'),
}


def make(size, content, style, near, samples, metric):
    plan = _hip.Plan(net, size, size)
    plan.set_style_nearest(near)
    if metric != 'l2':
        plan.set_nearest_metric(metric)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        if near[i]:
            tap = plan.feature(layer)[0].flatten(1)
            columns = _nearest_sample_columns(tap.shape[1], samples)
            plan.set_style_vectors(i, tap if len(columns) == tap.shape[1] else tap[:, torch.tensor(columns, device=DEV)])
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
    plans = {name: make(size, content, style, *arm) for name, arm in ARMS.items()}
    ms = {name: [] for name in plans}
    for _ in range(3):
        for name, plan in plans.items():
            ms[name].append(timed(plan, content))
    # the whole head alone at relu4_1: the iterate's tap against the style's, both finish passes behind the same search
    first = next(iter(plans.values()))
    first.forward(style, 29)
    vectors = first.feature(20)[0].flatten(1).contiguous()
    first.forward(content, 29)
    feat = first.feature(20)[0].contiguous()
    c, n, m = int(feat.shape[0]), int(feat.shape[1] * feat.shape[2]), int(vectors.shape[1])
    l2_set = _hip.op_nearest_prepare(vectors)
    cos_set = _hip.op_nearest_cosine_prepare(vectors, centered=True)
    head = {'shape': [c, n, m], 'splits': _hip.nearest_splits(n, m), 'l2_head_ms': [], 'cosine_head_ms': [], 'l2_search_ms': [],
            'cosine_search_ms': []}
    for _ in range(3):
        head['l2_search_ms'].append(events(lambda k: _hip.op_nearest_search(feat, l2_set, m), 3, 20))
        head['cosine_search_ms'].append(events(lambda k: _hip.op_nearest_search(feat, cos_set, m), 3, 20))
        head['l2_head_ms'].append(events(lambda k: _hip.op_nearest_loss(feat, l2_set, m), 3, 20))
        head['cosine_head_ms'].append(events(lambda k: _hip.op_nearest_cosine_loss(feat, cos_set, m), 3, 20))
    res['sizes'][str(size)] = {'ms': ms, 'relu4_1': head, 'device_bytes': {name: plan.device_bytes() for name, plan in plans.items()}}
    del plans, first
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
            head = entry['relu4_1']
            f.write(f'\n{size} x {size}, relu4_1 alone, C x N x M = {head["shape"][0]} x {head["shape"][1]} x {head["shape"][2]}, '
                    f'{head["splits"]} splits, best of three (ms): search + merge {min(head["l2_search_ms"]):.3f} on the L2 set, '
                    f'{min(head["cosine_search_ms"]):.3f} on the cosine set; the whole head {min(head["l2_head_ms"]):.3f} with the L2 '
                    f'finish, {min(head["cosine_head_ms"]):.3f} with the cosine finish\n\n')
print(json.dumps(res))

#!/usr/bin/env python3
"""Context for profiles/style_nearest.md, no pass / fail: milliseconds per plan.step on the default layers (content [22] as 'mse',
style [1, 6, 11, 20, 29]), at 128^2 and at 512^2, for
  fast                 five full W2 heads on the closure built for them,
  w2,w2,w2,gram,gram   the mixed list of profiles/layer_losses.md,
  w2,w2,w2,diag,diag   full W2 on the shallow heads, diagonal on relu4_1 / relu5_1,
  w2,w2,w2,near,near   full W2 on the shallow heads, nearest on relu4_1 / relu5_1 (Plan.set_style_nearest), every style vector,
  nearest-4096         five nearest heads, each against at most 4096 evenly spaced style vectors (style_nearest_samples = 4096).
Each: 10 warm-up steps, then 50 steps between two HIP events; the arms alternate three times in one process per size.  Then
the search launch alone at relu4_1 (st_op_nearest_search, whose second launch is the N-element merge) and the whole head
(st_op_nearest_loss), 20 calls between two events, with the search's rate on 6 C N M flop against the 833 TF fp16x3 peak.  Prints
one JSON line; --out FILE also writes it there and --markdown FILE writes the tables of profiles/style_nearest.md.

    python tools/style_nearest_ab.py [--out FILE] [--markdown FILE] [--sizes 128 512]
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
PEAK_TF = 833.0
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
STYLE = [1, 6, 11, 20, 29]
W2 = ['w2'] * 5
DEEP = [False, False, False, True, True]
ARMS = {                       # name: (style kinds, diagonal flags, nearest flags, samples)
    'w2,w2,w2,gram,gram': (['w2', 'w2', 'w2', 'gram', 'gram'], None, None, None),
    'w2,w2,w2,diag,diag': (W2, DEEP, None, None),
    'w2,w2,w2,near,near': (W2, None, DEEP, None),
    'nearest-4096': (W2, None, [True] * 5, 4096),
}


def make(size, content, style, kinds, diag, near, samples):
    plan = _hip.Plan(net, size, size)
    if kinds != W2:
        plan.set_layer_loss_kinds(['mse'], kinds)
    if diag is not None:
        plan.set_w2_diagonal(diag)
    if near is not None:
        plan.set_style_nearest(near)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        if near is not None and near[i]:
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
    default = make(size, content, style, W2, None, None, None)
    plans = {name: make(size, content, style, *arm) for name, arm in ARMS.items()}
    ms = {name: [] for name in ['fast', *plans]}
    for _ in range(3):
        ms['fast'].append(timed(default, content))
        for name, plan in plans.items():
            ms[name].append(timed(plan, content))
    # the search alone and the whole head at relu4_1: the iterate's tap against the style's
    default.forward(style, 29)
    vectors = default.feature(20)[0].flatten(1).contiguous()
    default.forward(content, 29)
    feat = default.feature(20)[0].contiguous()
    c, n, m = int(feat.shape[0]), int(feat.shape[1] * feat.shape[2]), int(vectors.shape[1])
    prepared = _hip.op_nearest_prepare(vectors)
    search_ms = events(lambda k: _hip.op_nearest_search(feat, prepared, m), 3, 20)
    head_ms = events(lambda k: _hip.op_nearest_loss(feat, prepared, m), 3, 20)
    res['sizes'][str(size)] = {
        'ms': ms,
        'relu4_1': {'shape': [c, n, m], 'splits': _hip.nearest_splits(n, m), 'search_ms': search_ms, 'head_ms': head_ms,
                    'search_tf': 6.0 * c * n * m / (search_ms * 1e-3) / 1e12,
                    'search_fraction_of_peak': 6.0 * c * n * m / (search_ms * 1e-3) / 1e12 / PEAK_TF},
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
            head = entry['relu4_1']
            f.write(f'\n{size} x {size}, relu4_1 alone, C x N x M = {head["shape"][0]} x {head["shape"][1]} x {head["shape"][2]}, '
                    f'{head["splits"]} splits: search + merge {head["search_ms"]:.3f} ms ({head["search_tf"]:.1f} TF on 6 C N M flop, '
                    f'{100 * head["search_fraction_of_peak"]:.1f} % of {PEAK_TF:.0f} TF), the whole head {head["head_ms"]:.3f} ms\n\n')
print(json.dumps(res))

#!/usr/bin/env python3
"""Context for profiles/w2_marginal.md, no pass / fail: milliseconds per plan.step on the default layers (content [22] as 'mse',
style [1, 6, 11, 20, 29]), at 128^2 and at 512^2, for
  fast                 five full W2 heads on the closure built for them,
  gram                 five Gram heads (Plan.set_layer_loss_kinds),
  w2,w2,w2,gram,gram   the mixed list of profiles/layer_losses.md,
  diagonal             five diagonal W2 heads (Plan.set_w2_diagonal),
  w2,w2,w2,diag,diag   full W2 on the shallow heads, diagonal on relu4_1 / relu5_1,
  marginal             five marginal heads (Plan.set_w2_marginal), a chunk of 4096 keys per workgroup of the sort,
  marginal-8192        the same plan under ST_SORT_CHUNK=8192 (st_set_option),
  w2,w2,w2,marg,marg   full W2 on the shallow heads, marginal on relu4_1 / relu5_1.
Each: 10 warm-up steps, then 50 steps between two HIP events; the arms alternate three times in one process per size.  Then,
per style layer, the marginal head's launches alone on that layer's tap (st_op_w2_marginal_loss: the sort's launches and the
residual pass; st_op_channel_sort without outputs: the sort alone), 20 calls between two events, for both chunk sizes.  Prints
one JSON line; --out FILE also writes it there and --markdown FILE writes the tables of profiles/w2_marginal.md.

    python tools/w2_marginal_ab.py [--out FILE] [--markdown FILE] [--sizes 128 512]
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
ap.add_argument('--sizes', type=int, nargs='+', default=[128, 512])
args = ap.parse_args()
DEV = 'cuda:0'
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', DEV, 'fp16x3')
STYLE = [1, 6, 11, 20, 29]
W2 = ['w2'] * 5
DEEP = [False, False, False, True, True]
ARMS = {                       # name: (style kinds, diagonal flags, marginal flags)
    'gram': (['gram'] * 5, None, None),
    'w2,w2,w2,gram,gram': (['w2', 'w2', 'w2', 'gram', 'gram'], None, None),
    'diagonal': (W2, [True] * 5, None),
    'w2,w2,w2,diag,diag': (W2, DEEP, None),
    'marginal': (W2, None, [True] * 5),
    'w2,w2,w2,marg,marg': (W2, None, DEEP),
}


def make(size, content, style, kinds, diag, marg):
    plan = _hip.Plan(net, size, size)
    if kinds != W2:
        plan.set_layer_loss_kinds(['mse'], kinds)
    if diag is not None:
        plan.set_w2_diagonal(diag)
    if marg is not None:
        plan.set_w2_marginal(marg)
    plan.forward(content, 29)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate(STYLE):
        if marg is not None and marg[i]:
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


def timed(plan, content, chunk=4096):
    x = content.clone()
    m, v, e = torch.zeros_like(x), torch.zeros_like(x), 0.01 * x
    with _hip.options(ST_SORT_CHUNK=chunk):
        return events(lambda k: plan.step(x, m, v, e, k + 1, 0.02), 10, 50)


res = {'device': torch.cuda.get_device_name(0), 'sizes': {}}
for size in args.sizes:
    gen = torch.Generator().manual_seed(3)
    content = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    style = torch.rand((1, 3, size, size), generator=gen).to(DEV)
    default = make(size, content, style, W2, None, None)
    plans = {name: make(size, content, style, *arm) for name, arm in ARMS.items()}
    ms = {name: [] for name in ['fast', *plans, 'marginal-8192']}
    for _ in range(3):
        ms['fast'].append(timed(default, content))
        for name, plan in plans.items():
            ms[name].append(timed(plan, content))
        ms['marginal-8192'].append(timed(plans['marginal'], content, chunk=8192))
    # the marginal head's launches alone, per layer, for both chunk sizes
    plans['marginal'].forward(content, 29)
    heads = {}
    for layer in STYLE:
        feat = plans['marginal'].feature(layer)[0].contiguous()
        target = _hip.op_channel_sort(plans['diagonal'].feature(layer)[0].contiguous(), indices=False)[0]
        entry = {'shape': [int(feat.shape[0]), int(feat.shape[1] * feat.shape[2])]}
        for chunk in (4096, 8192):
            with _hip.options(ST_SORT_CHUNK=chunk):
                entry[f'sort_ms_{chunk}'] = events(lambda k: _hip.op_channel_sort(feat, values=False, indices=False), 3, 20)
                entry[f'head_ms_{chunk}'] = events(lambda k: _hip.op_w2_marginal_loss(feat, target), 3, 20)
        heads[str(layer)] = entry
    res['sizes'][str(size)] = {
        'ms': ms,
        'heads': heads,
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
            f.write(f'\n{size} x {size}, one marginal head alone, ms per call (sort / sort + residual):\n\n')
            f.write('| layer | C x N | chunk 4096 | chunk 8192 |\n|---|---|---|---|\n')
            for layer, head in entry['heads'].items():
                f.write(f'| features[{layer}] | {head["shape"][0]} x {head["shape"][1]} | {head["sort_ms_4096"]:.3f} / '
                        f'{head["head_ms_4096"]:.3f} | {head["sort_ms_8192"]:.3f} / {head["head_ms_8192"]:.3f} |\n')
            f.write('\n')
print(json.dumps(res))

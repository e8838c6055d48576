#!/usr/bin/env python3
"""A/B of the reference's module closure on this package, in one process:

    feats = model(image); loss = crit(feats); loss.backward()          (reference style_transfer.py:472-476)

with `model` = VGGFeatures (the HIP trunk) and `crit` = the reference's SumLoss graph on the default layers and losses
(ContentLossMSE at 22, StyleLossW2 at 1 6 11 20 29, TVLoss; reference :376,427-455).  Arm "native": the loss modules on the
library's standalone heads and pointwise entries (style_transfer/losses.py).  Arm "torch": the same graph under
losses.native(False) - the modules' torch code on the same trunk.  The arms alternate, every arm is warmed up and timed
over at least `--seconds` of closures closed by a device synchronise.  For orientation, the same targets through
plan.loss_and_grad on the general closure (ST_GENERAL_TAPS=1), which runs the same terms inside the library.

    python tools/native_losses_ab.py [--sizes 128 512] [--repeats 3] [--seconds 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, 'style-transfer-pytorch_amd'))
sys.path.insert(0, os.path.join(R, 'tests'))
import torch
import synth
from style_transfer import _hip, losses, vgg
from style_transfer.style_transfer import (ContentLossMSE, LayerApply, Scale, StyleLossW2, SumLoss, TVLoss, VGGFeatures)

DEV = 'cuda:0'
WARMUP = 10
STYLE_LAYERS, STYLE_WEIGHTS = [1, 6, 11, 20, 29], [w / 341 for w in (256, 64, 16, 4, 1)]


def make_graph(model, content, style):
    with torch.no_grad():
        cfeat = model(content, layers=[22])[22]
        feats = model(style, layers=STYLE_LAYERS)
        moments = {layer: StyleLossW2.get_target(feats[layer]) for layer in STYLE_LAYERS}
    members = [Scale(LayerApply(ContentLossMSE(cfeat), 22), 0.015)]
    members += [Scale(LayerApply(StyleLossW2(moments[layer]), layer), w) for layer, w in zip(STYLE_LAYERS, STYLE_WEIGHTS)]
    members.append(Scale(LayerApply(TVLoss(), 'input'), 2.0))
    return SumLoss(members).to(DEV), cfeat, moments


class ModuleArm:
    def __init__(self, model, crit, image, native):
        self.model, self.crit, self.native = model, crit, native
        self.image = image.clone().requires_grad_(True)

    def iterate(self):
        with losses.native(self.native):
            self.image.grad = None
            loss = self.crit(self.model(self.image))
            loss.backward()
        return loss


class PlanArm:
    def __init__(self, model, size, cfeat, moments, image):
        self.plan = _hip.Plan(model.net, size, size)
        self.plan.set_content_target(cfeat[0])
        for i, layer in enumerate(STYLE_LAYERS):
            self.plan.set_style_target(i, moments[layer][0][0], moments[layer][1][0])
        self.plan.set_loss_weights(0.015, STYLE_WEIGHTS, 2.0)
        self.image, self.grad = image.clone(), torch.empty_like(image)

    def iterate(self):
        with _hip.options(ST_GENERAL_TAPS=1):
            return self.plan.loss_and_grad(self.image, self.grad)[0]


def timed(arm, seconds):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        arm.iterate()
        n += 1
        if n % 8 == 0 and time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--out')
    a = ap.parse_args()
    model = VGGFeatures(STYLE_LAYERS + [22], 'max', weights=vgg.synthetic_vgg19_weights(0), device=DEV, precision='fp16x3')
    results = {'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for size in a.sizes:
        content = synth.smooth_image(21, size, size).to(DEV)
        style = synth.smooth_image(22, size, size).to(DEV)
        crit, cfeat, moments = make_graph(model, content, style)
        arms = {'torch': ModuleArm(model, crit, content, False), 'native': ModuleArm(model, crit, content, True),
                'plan': PlanArm(model, size, cfeat, moments, content)}
        for arm in arms.values():
            for _ in range(WARMUP):
                arm.iterate()
        rates = {k: [] for k in arms}
        for _ in range(a.repeats):
            for k, arm in arms.items():
                rates[k].append(timed(arm, a.seconds))
        t, n, p = rates['torch'], rates['native'], rates['plan']
        verdict = 'native faster in every repeat' if min(n) > max(t) else 'NOT faster in every repeat'
        print(f'{size}^2: torch modules {" ".join(f"{v:.1f}" for v in t)} closures/s (spread {(max(t) - min(t)) / min(t):.1%}); '
              f'native modules {" ".join(f"{v:.1f}" for v in n)} (spread {(max(n) - min(n)) / min(n):.1%}); '
              f'slowest native / fastest torch = {min(n) / max(t):.3f}: {verdict}; '
              f'plan.loss_and_grad (general closure) {" ".join(f"{v:.1f}" for v in p)}', flush=True)
        results['sizes'][str(size)] = {'torch': t, 'native': n, 'plan_general': p, 'slowest_native_over_fastest_torch': min(n) / max(t)}
        del arms, crit
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Headline benchmark: optimiser iterations/sec of the style-transfer hot loop on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--size S | WxH] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-extra] [--no-pmc]]

One "step" = one full iteration of reference style_transfer.py:479-486 (VGG-19 forward, 7-term loss,
backward to the pixels, Adam, clamp, EMA), synthetic seeded content/style images and seeded synthetic
VGG-19 weights (no network, no pretrained file in this image).  All inputs are resident in HBM before the
timed region.

A plain run sets up, runs W warm-up steps, times K steps (`value`, `ms_per_step`), writes the last timed step's
outputs when --dump-outputs is given, and prints its line.  Everything else the benchmark measures runs only with
--full: two more K-step regions (`value_regions`, `value_best_of_3`), the profiled steps of `roofline` /
`roofline_hbm`, and at N = 1 the items below.

* N = 1 (default): a 512 x 512 image - the end scale of BASELINE.json configs[1], the config the metric is
  quoted on.  With --full the line also carries `extra_sizes` (short runs at 1024^2, 2048^2 and 2896x2172 on the
  same GPU: the single-GPU points of configs[2..4]), the other conv arithmetic modes, `config2_default_run` and
  `cpu_baseline` (the unmodified reference's --devices cpu path, staged by oracle/make_ref.py, timed with its own
  STIterate.time hook on the host cores).
* N > 1: the driver launches one rank per GPU (torch.distributed, backend nccl = RCCL) and ONE 2048 x 2048 image
  (configs[3]; `--size` overrides) is cut into N row strips - halo exchange + Gram all-reduce, "scaling":
  "strong", `value` = iterations/s of that image.  The strong-scaling base is `extra_sizes["2048x2048"]` of the
  N = 1 line.  `--scaling weak` (one size x size strip per GPU) and `--mode replicas` remain as options.  If the
  sharded path fails the line says so with "value": null and the exit code is 1 - there is no silent fallback.

Rank 0 prints ONE JSON line.

--dump-outputs DIR: what a caller of the timed path receives after the last timed step - the image, its EMA, the two
Adam moments and the 8 loss values (7 weighted terms + total) - as DIR/<name>.npy (float32), the strips of a sharded
run joined into the whole image.  At most 64 MiB in all: above that, larger arrays are replaced by a fixed seeded
sample of their elements.  The inputs are seeded, so two builds run with the same arguments can be compared file by file.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, 'style-transfer-pytorch_amd'))

PEAK_HBM_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E ~8 TB/s (spec; ~6.3 TB/s achievable)
PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA
# algorithmic (fp32-equivalent) FLOP peak of the conv kernel per arithmetic mode: one useful MAC costs
# 1 fp32 MFMA MAC, or 6 / 3 bf16 MFMA MACs in the split-precision modes
MFMA_PRODUCTS = {'fp16x3': 3, 'bf16x3': 3, 'bf16x6': 6}      # 16-bit MFMA MACs executed per algorithmic MAC (direct kernels)
CONV_PEAK = {'fp32': PEAK_FP32_MFMA_TFLOPS, 'bf16x6': PEAK_BF16_MFMA_TFLOPS / 6, 'bf16x3': PEAK_BF16_MFMA_TFLOPS / 3,
             'fp16x3': PEAK_BF16_MFMA_TFLOPS / 3}
CONV_MODE = {'fp32': 'exact fp32 MFMA (v_mfma_f32_32x32x2_f32)',
             'bf16x6': 'split-precision bf16 MFMA: 3 bf16 planes per fp32 operand, 6 products, fp32 accumulate '
                       '(fp32-class accuracy; passes the fp32 parity tests unchanged)',
             'bf16x3': 'split-precision bf16 MFMA: 2 planes, 3 products (APPROXIMATE: gradient rel-L2 ~2e-3)',
             'fp16x3': 'split-precision fp16 MFMA: 2 fp16 planes per fp32 operand (22 significant bits, power-of-two '
                       'per-tensor scaling measured on device), 3 products, fp32 accumulate (fp32-class accuracy; '
                       'passes the fp32 parity tests unchanged)'}
# `dtype` = the arithmetic the path computes in: every tensor in HBM, every accumulator and every non-conv kernel is
# fp32; the twelve 3x3 trunk convolutions multiply fp32 operands as split 16-bit planes on the MFMA (fp32 accumulate)
DTYPE_LABEL = {'fp32': 'f32', 'fp16x3': 'f32 (3x3 convs: fp16x3 split-plane MFMA, fp32 accumulate)',
               'bf16x6': 'f32 (3x3 convs: bf16x6 split-plane MFMA, fp32 accumulate)',
               'bf16x3': 'f32 storage, bf16x3 conv products (approximate)'}
CONV_SPECS = [(3, 64, 0), (64, 64, 0), (64, 128, 1), (128, 128, 1), (128, 256, 2), (256, 256, 2), (256, 256, 2),
              (256, 256, 2), (256, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 3), (512, 512, 4)]


def conv_flops(h, w):
    """forward + data-gradient FLOPs of the 13 convolutions."""
    return 2 * sum(2 * 9 * ci * co * (h >> p) * (w >> p) for ci, co, p in CONV_SPECS)


def conv_algorithmic_bytes_per_launch(h, w):
    """Mean unavoidable HBM bytes of one 3x3 trunk conv launch (the 12 MFMA layers, forward and data gradient): its
    fp32 operand read once, its fp32 result written once, its pre-split weights (2 fp16 planes = 4 B / weight)."""
    tot = 0
    for ci, co, p in CONV_SPECS[1:]:
        px = (h >> p) * (w >> p)
        tot += 2 * ((ci + co) * px * 4 + 9 * ci * co * 4)
    return tot / (2 * len(CONV_SPECS[1:]))


def conv_fused_path_bytes_per_launch(h, w):
    """The same mean, counting what the closure's launches really have to move: the data-gradient launches also apply
    threshold_backward (they read the ReLU output of the map they write - not where that map is a pooled one, whose mask
    bit travels in the argmax codes) and add the style / content heads' gradients at the five taps they land on
    (relu1_1, 2_1, 3_1, 4_1, 4_2: one more read of the map); the four forward launches in front of a max pool write the
    pooled map plus one byte per window instead of the full-resolution map."""
    tot = 0
    layers = CONV_SPECS[1:]
    pooled_after = {1, 3, 7, 11}           # conv1_2, 2_2, 3_4, 4_4 (index into CONV_SPECS)
    input_is_pooled = {2, 4, 8, 12}        # conv2_1, 3_1, 4_1, 5_1
    input_is_tap = {1, 3, 5, 9, 10}        # conv1_2, 2_2, 3_2, 4_2, 4_3
    for k, (ci, co, p) in enumerate(layers, start=1):
        px = (h >> p) * (w >> p)
        wb = 9 * ci * co * 4
        tot += ci * px * 4 + (co * (px // 4) * 5 if k in pooled_after else co * px * 4) + wb          # forward
        tot += co * px * 4 + ci * px * 4 + wb                                                          # data gradient
        tot += (0 if k in input_is_pooled else ci * px * 4) + (ci * px * 4 if k in input_is_tap else 0)
    return tot / (2 * len(layers))


def synthetic_image(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, max(h // 16, 2), max(w // 16, 2)), generator=g)
    img = torch.nn.functional.interpolate(low, (h, w), mode='bicubic', align_corners=False)
    img = img + (torch.rand((1, 3, h, w), generator=g) - 0.5) * (24 / 255)
    return img.clamp(0, 1).contiguous()


def cpu_baseline(size, budget_s=30.0):
    """The reference's --devices cpu path on this box's host cores (rank 0, N = 1 only).

    kind "reference": the UNMODIFIED reference (oracle/_ref, staged by oracle/make_ref.py in the build container)
    through oracle/ref_runner.py - its own stylize() loop, timed by its own STIterate.time stamps (BASELINE.md
    section 3).  kind "port": the oracle (oracle/st_oracle.py) when the staged copy is absent.  A bounded sample: a
    few iterations per OpenMP thread count (16, 32, 8, 64 - never more than the CPUs the container may use), the
    best one reported.  Runs as a CHILD process with a hard wall-clock limit, so a pathological host (thread
    oversubscription made one round-1 iteration take minutes) cannot stall the benchmark."""
    import subprocess
    cmd = [sys.executable, os.path.join(REPO, 'oracle', 'ref_runner.py'), '--size', str(size), '--threads', '16,32,8,64',
           '--budget', str(budget_s)]
    t0 = time.perf_counter()
    try:
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=budget_s + 40, text=True)
        text, note = proc.stdout, None if proc.returncode == 0 else f'child exited with {proc.returncode}'
    except subprocess.TimeoutExpired as exc:
        text = exc.stdout.decode() if isinstance(exc.stdout, bytes) else (exc.stdout or '')
        note = f'child killed at the {budget_s + 40:.0f} s wall-clock limit'
    head, runs = {}, []
    for line in text.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if 'threads' in rec:
            runs.append(rec)
        else:
            head.update(rec)
    runs = [r for r in runs if r.get('timed_iterations', 0) > 0]
    if not runs:
        return {'value': None, 'unit': 'it/s', 'cores': None, 'kind': head.get('kind', 'reference'),
                'sample': f'no timed iteration completed ({note})'}
    best = max(runs, key=lambda r: r['it_s'])
    kind = head.get('kind', 'reference')
    what = ('unmodified reference stylize(), min_scale = end_scale = %d, devices=[cpu], median of STIterate.time '
            'differences after dropping the first two iterations' % size) if kind == 'reference' else \
        'oracle/st_oracle.py iterate() (port of the reference loop), median iteration time after 1 warm-up'
    out = {'value': best['it_s'], 'unit': 'it/s', 'cores': best['threads'], 'kind': kind,
           'sample': f'{what}; {best["timed_iterations"]} timed iterations at the best of {len(runs)} thread counts '
                     f'({time.perf_counter() - t0:.1f} s of CPU work in total)',
           'threads_sweep_it_s': {str(r['threads']): round(r['it_s'], 4) for r in runs},
           'host_hw_threads': head.get('hw_threads'), 'usable_cpus': head.get('usable_cpus')}
    if note:
        out['note'] = note
    return out


def parse_size(text):
    """'512' -> (512, 512) (height, width); '2896x2172' (W x H as the reference's CLI prints sizes) -> (2172, 2896)."""
    if 'x' in str(text):
        w, h = str(text).lower().split('x')
        return int(h), int(w)
    return int(text), int(text)


def run_single(args, dev, rank, world, hw=None):
    """N == 1 (or replicas): the whole image on this GPU, fused st_plan_step per iteration."""
    from style_transfer import _hip, vgg
    height, width = hw or (args.height, args.width)
    weights = vgg.synthetic_vgg19_weights(0)
    content = synthetic_image(100 + rank, height, width)
    style = synthetic_image(200 + rank, height, width)
    image0 = content.clone()                               # init='content' (reference default)
    net = _hip.Net(weights, 'max', dev, args.precision)
    plan = _hip.Plan(net, height, width)
    plan.forward(content.to(dev), 22)
    plan.set_content_target_from_forward()
    plan.forward(style.to(dev), 29)
    for i, layer in enumerate([1, 6, 11, 20, 29]):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    image = image0.to(dev).clone()
    m, v = torch.zeros_like(image), torch.zeros_like(image)
    ema = (1 - torch.tensor(0.99)).to(dev) * image
    state = {'step': 0}

    def step():
        state['step'] += 1
        plan.step(image, m, v, ema, state['step'], 0.02)
    step.outputs = lambda: {'image': image, 'image_ema': ema, 'adam_exp_avg': m, 'adam_exp_avg_sq': v, 'losses': plan.losses}
    return plan, step, (weights, content, style, image0), (lambda: float(plan.losses[7].item()))


def sharded_shape(args, world):
    """Global image of the sharded run.  weak (default): one size x size strip per rank, i.e. a (size * N) x size
    image - per-GPU work is fixed as N grows; strong: the same size x size image cut into N strips."""
    return (args.height * world if args.scaling == 'weak' else args.height), args.width


def run_sharded(args, dev, rank, world, conservative=False, native=False):
    """N > 1: one strip of the SAME image per rank; halo exchange + Gram reduction over RCCL.  conservative=True: the
    fallback form - whole convolution launches, every rank runs every Newton-Schulz chain on all-reduced moments, and
    every exchange bracketed by device-wide synchronisation (no stream-ordered communication)."""
    from style_transfer import _hip, sharding, vgg
    if not conservative and os.environ.get('ST_BENCH_INJECT_FAILURE') in ('all', str(rank)):
        raise RuntimeError('injected failure (ST_BENCH_INJECT_FAILURE: exercises the fallback to the conservative transport)')
    if conservative:
        _hip.set_option('ST_STRIP_OVERLAP', 0)
        _hip.set_option('ST_STRIP_NS_OWNER', 0)
    height, width = sharded_shape(args, world)
    weights = vgg.synthetic_vgg19_weights(0)
    content = synthetic_image(100, height, width)          # every rank draws the same global images
    style = synthetic_image(200, height, width)
    b, e = sharding.strip_rows(height, world, width)[rank]
    net = _hip.Net(weights, 'max', dev, args.precision)
    plan = sharding.StripPlan(net, height, width, b, e).set_rank(rank, world)
    fabric = sharding.DistFabric(rank, world, host_sync=True if conservative else None)
    if native:
        # the in-library transport (csrc/st_fabric.hip): RCCL operations issued by the library on its own streams, the whole
        # phase sequence in one call; torch.distributed (the DistFabric above) only carries the cold path
        fabric = sharding.NativeFabric(rank, world, dev, cold=fabric)
    cstrip = content[:, :, b:e].contiguous().to(dev)
    sstrip = style[:, :, b:e].contiguous().to(dev)
    sharding.set_targets(plan, cstrip, [sstrip], [1.0], lambda p: sharding.run_phases(p, fabric), fabric.allreduce)
    plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)
    image = cstrip.clone()
    grad = torch.empty_like(image)
    m, v = torch.zeros_like(image), torch.zeros_like(image)
    ema = (1 - torch.tensor(0.99)).to(dev) * image
    state = {'step': 0}

    def step():
        state['step'] += 1
        plan.closure_begin(image, grad)
        sharding.run_phases(plan, fabric)
        plan.apply_update(image, grad, m, v, ema, state['step'], 0.02)
    step.fabric = fabric
    step.outputs = lambda: {'image': image, 'image_ema': ema, 'adam_exp_avg': m, 'adam_exp_avg_sq': v, 'losses': plan.losses}
    return plan, step, None, (lambda: float(plan.losses[7].item()))


def first_iteration(step, dev, native):
    """The first full iteration of a sharded attempt, awaited on the HOST with a deadline: a transport that deadlocks
    (a phase-order mismatch between ranks, a fabric problem the pre-flight did not show) must end as a failed attempt the
    next transport can replace, not as a bench that never prints its line.  In-library transport: its communicators are
    aborted (ncclCommAbort ends the kernels in flight), the queued work drains, and the caller moves on.
    ST_BENCH_FIRST_STEP_S (default 120); ST_BENCH_INJECT_FAILURE=deadline gives the in-library attempt a deadline of 0."""
    deadline = float(os.environ.get('ST_BENCH_FIRST_STEP_S', '120'))
    if native and os.environ.get('ST_BENCH_INJECT_FAILURE') == 'deadline':
        deadline = 0.0
    step()
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    t0 = time.perf_counter()
    while not done.query():
        if time.perf_counter() - t0 > deadline:
            fabric = getattr(step, 'fabric', None)
            if native and fabric is not None:
                fabric.close(abort=True)
                torch.cuda.synchronize(dev)              # what was queued behind the aborted operations drains
            raise TimeoutError(f'the first sharded iteration did not complete within {deadline:g} s')
        time.sleep(0.002)


PMC_TRAFFIC_FILES = ('r04_pmc_traffic_conv.json', 'r03_pmc_traffic_conv.json', 'r02_pmc_traffic_conv.json')


def pmc_traffic(args, prec, mode):
    """(bytes, provenance): HBM-side bytes per conv launch from the newest committed rocprofv3 PMC passes
    (tools/pmc_traffic.sh: FETCH_SIZE and WRITE_SIZE in separate runs, gfx950 correction applied).  Counters cannot be
    read inside this process, so the figure is REPLAYED from profiles/ and labelled as such - and only for the
    configuration it was taken on (512^2, fp16x3, one GPU); (None, reason) otherwise."""
    if (args.height, args.width) != (512, 512) or prec != 'fp16x3' or mode != 'single':
        return None, 'no PMC pass exists for this configuration (taken at 512x512, fp16x3, single GPU only)'
    for name in PMC_TRAFFIC_FILES:
        path = os.path.join(REPO, 'profiles', name)
        if os.path.exists(path):
            with open(path) as f:
                rec = json.load(f)
            return rec['hbm_side_bytes_per_launch'], {
                'replayed_from': 'profiles/' + name, 'measured_in_this_run': False,
                'collected': rec.get('collected', 'round ' + name[1:3] + ' gpurun box (MI355X), tools/pmc_traffic.sh'),
                'kernels': rec.get('kernels', 'conv_pc_kernel / conv_fat_kernel / conv_split_kernel launches of bench.py --steps 20')}
    return None, 'profiles/*_pmc_traffic_conv.json not found'


PMC_KERNELS = ('conv_split_kernel', 'conv_pc_kernel', 'conv_fat_kernel')


def pmc_traffic_measured(args, prec, mode):
    """HBM-side bytes per conv launch MEASURED for this run: two child runs of this script under
    `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `... WRITE_SIZE` (separate passes, as MI355X_MICROARCH.md prescribes; 3 + 2
    iterations each, no extras), FETCH_SIZE x 2 (gfx950: wide coalesced reads are counted at half) + WRITE_SIZE over the 3 x 3
    trunk launches.  Counters cannot be read inside this process.  (None, reason) when rocprofv3 is not there, a pass fails or
    takes longer than 150 s - the caller then falls back to the replayed figure and says so."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if mode != 'single' or os.environ.get('ST_BENCH_PMC_CHILD') == '1':
        return None, 'not an N = 1 single-image run'
    exe = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if exe is None:
        return None, 'rocprofv3 not found'
    size = f'{args.width}x{args.height}'
    got = {}
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory(dir='/tmp') as tmp:
        for counter, sub in (('FETCH_SIZE', 'f'), ('WRITE_SIZE', 'w')):
            cmd = [exe, '--kernel-trace', '--pmc', counter, '-d', os.path.join(tmp, sub), '-o', sub, '--output-format', 'csv', '--',
                   sys.executable, os.path.abspath(__file__), '--size', size, '--steps', '3', '--warmup', '2', '--precision', prec,
                   '--no-cpu-baseline', '--no-extra', '--no-pmc', '--full']
            env = dict(os.environ, TMPDIR='/tmp', ST_BENCH_PMC_CHILD='1')
            try:
                r = subprocess.run(cmd, cwd='/tmp', env=env, capture_output=True, text=True, timeout=150)
            except subprocess.TimeoutExpired:
                return None, f'the {counter} pass did not finish within 150 s'
            files = glob.glob(os.path.join(tmp, sub, '**', '*counter_collection.csv'), recursive=True)
            if r.returncode != 0 or not files:
                return None, f'the {counter} pass failed (rc {r.returncode}): {(r.stderr or r.stdout)[-200:]}'
            tot, n = 0.0, 0
            with open(files[0]) as f:
                for row in csv.DictReader(f):
                    if row['Counter_Name'] == counter and any(k in row['Kernel_Name'] for k in PMC_KERNELS):
                        tot += float(row['Counter_Value'])
                        n += 1
            if n == 0:
                return None, f'the {counter} pass saw no convolution launch'
            got[counter] = (tot / n, n)
    kb = 2 * got['FETCH_SIZE'][0] + got['WRITE_SIZE'][0]
    return kb * 1024, {'measured_in_this_run': True, 'method': 'two child runs of bench.py under rocprofv3 --kernel-trace --pmc '
                       'FETCH_SIZE / WRITE_SIZE (3 + 2 iterations each); FETCH_SIZE x 2 + WRITE_SIZE, KB -> bytes, mean over the '
                       'conv_pc_kernel / conv_fat_kernel / conv_split_kernel launches',
                       'launches_sampled': got['FETCH_SIZE'][1], 'FETCH_SIZE_KB_per_launch_raw': got['FETCH_SIZE'][0],
                       'WRITE_SIZE_KB_per_launch_raw': got['WRITE_SIZE'][0], 'seconds': time.perf_counter() - t0}


def hbm_rooflines(plan, prof_steps):
    """Achieved GB/s of the step's HBM-bound kernels: algorithmic bytes (operands read once + results written once)
    / HIP-event time of each launch on its own stream, against 8 TB/s."""
    out = {}
    for name, (n, ms, nbytes) in plan.profile_read_hbm().items():
        if n == 0 or ms <= 0:
            continue
        gbs = nbytes / (ms * 1e-3) / 1e9
        out[name] = {'bound': 'hbm', 'achieved': gbs, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': gbs / PEAK_HBM_GBS,
                     'launches_per_step': n / prof_steps, 'avg_launch_us': ms * 1e3 / n,
                     'algorithmic_mb_per_launch': nbytes / n / 1e6}
        if name.startswith('Adam'):
            # (the TIMED steps have no such launch: st_plan_step lets conv1_1's fold kernel apply the update - ST_STEP_TAIL=2;
            # the profiled steps keep the separate kernel so that it can be timed)
            out[name]['note'] = 'profiled steps only; in the timed steps the update rides in conv1_1\'s fold kernel'
    return out


def timed_run(step, steps, warmup, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps


DUMP_LIMIT_BYTES = 64 * 2 ** 20


def write_outputs(path, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: each array as path/<name>.npy, float32 (float64 stays float64).  When together they hold more than
    `limit` bytes (npy headers included), the smaller arrays are written whole and every array larger than its share of
    what is left becomes a fixed sample of its flattened elements: indices drawn by a numpy Generator seeded with `seed`,
    in ascending order - the same elements from run to run.  Returns {name: (elements written, elements in the array)}."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64 if v.dtype == np.float64 else np.float32).reshape(v.shape)
              for k, v in arrays.items()}
    header = 4096                                     # bytes reserved per file for the npy header (<= 4 KiB when flattened)
    budget = limit - header * len(arrays)
    written = {}
    order = sorted(arrays, key=lambda k: (arrays[k].nbytes, k))
    for i, name in enumerate(order):
        a = arrays[name]
        share = budget // (len(order) - i)
        if a.nbytes > share:
            k = share // a.itemsize
            idx = np.sort(np.random.default_rng(seed).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + '.npy'), a)
        budget -= a.nbytes
        written[name] = (a.size, arrays[name].size)
    return written


def collect_outputs(step, mode, world):
    """The last step's outputs on the host (every rank takes part; what rank 0 returns is what it writes).  Sharded runs:
    each rank holds one row strip of the image and its state, joined here in rank order; the losses are the whole image's
    on every rank."""
    arrays = {k: t.detach().cpu().numpy() for k, t in step.outputs().items()}
    if mode == 'shard' and world > 1:
        import numpy as np
        import torch.distributed as dist
        parts = [None] * world
        dist.all_gather_object(parts, {k: v for k, v in arrays.items() if k != 'losses'})
        for k in parts[0]:
            arrays[k] = np.concatenate([p[k] for p in parts], axis=2)
    return arrays


def extra_sizes(args, dev):
    """Short single-GPU runs of the same hot loop at the larger BASELINE sizes (configs[2..4]'s N = 1 points)."""
    res = {}
    for text, steps in (('1024', 20), ('2048', 10), ('2896x2172', 8)):
        hw = parse_size(text)
        plan, step, _, read_loss = run_single(args, dev, 0, 1, hw)
        sec = timed_run(step, steps, 3, dev)
        plan.profile_enable(True)
        for _ in range(5):               # (2 profiled steps gave 318 ... 362 TF for the same build at 1024^2 from run to run)
            step()
        hbm = hbm_rooflines(plan, 5)
        launches, ms, flops = plan.profile_read()
        plan.profile_enable(False)
        conv_tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        final_loss = read_loss()
        # a kernel that skipped work would still print a time: the loss after these iterations is reported (and must be
        # a finite positive number) so that the entry can be compared run to run
        assert final_loss == final_loss and 0 < final_loss < 1e3, f'{text}: loss {final_loss}'
        res[f'{hw[1]}x{hw[0]}'] = {'it_s': 1.0 / sec, 'ms_per_step': sec * 1e3, 'steps': steps,
                                   'final_loss': final_loss, 'iterations_run': 3 + steps + 5,
                                   'conv_tflops': conv_tf, 'conv_roofline_frac': conv_tf / CONV_PEAK[args.precision],
                                   'whole_step_conv_tflops': conv_flops(*hw) / sec / 1e12,
                                   'roofline_hbm': hbm,
                                   'plan_device_gib': plan.device_bytes() / 2 ** 30}
        del plan, step
        torch.cuda.empty_cache()
    # HBM-side traffic of the conv launches at 2048^2 (where traffic matters): MEASURED in this run (two child runs under
    # rocprofv3 --pmc, like the headline's `roofline.traffic`) when rocprofv3 is there and the passes finish
    # in time, else replayed from the newest committed pass and labelled as such
    if '2048x2048' in res:
        import copy
        a2 = copy.copy(args)
        a2.height = a2.width = 2048
        measured, src = (None, 'PMC child passes disabled (--no-pmc)') if getattr(args, 'no_pmc', False) else \
            pmc_traffic_measured(a2, args.precision, 'single')
        entry = {'algorithmic_bytes_per_launch': conv_algorithmic_bytes_per_launch(2048, 2048),
                 'algorithmic_fused_path_bytes_per_launch': conv_fused_path_bytes_per_launch(2048, 2048)}
        if measured is not None:
            entry.update(bytes_per_launch=measured, source=src, measured_in_this_run=True)
        else:
            for name in ('r05_pmc_traffic_conv_2048.json', 'r04_pmc_traffic_conv_2048.json'):
                path = os.path.join(REPO, 'profiles', name)
                if os.path.exists(path):
                    with open(path) as f:
                        rec = json.load(f)
                    entry.update(bytes_per_launch=rec['hbm_side_bytes_per_launch'], replayed_from='profiles/' + name,
                                 measured_in_this_run=False, not_measured_because=src)
                    break
        if 'bytes_per_launch' in entry:
            entry['vs_algorithmic'] = entry['bytes_per_launch'] / entry['algorithmic_bytes_per_launch']
            res['2048x2048']['conv_traffic'] = entry
    return res


def config2_scales(args, dev, end_its):
    """BASELINE configs[1] as the CLI runs it ("report it/s per scale"): end_scale 512 with the
    defaults is the pyramid 128, 181, 256, 362, 512 with 1000 + 4 x 500 iterations (style_transfer.py:366-369,469).
    Short runs of the hot loop at the smaller scales; the 512^2 figure is the timed region's own."""
    res, total = {}, 0.0
    for size, its in ((128, 1000), (181, 500), (256, 500), (362, 500)):
        plan, step, _, _ = run_single(args, dev, 0, 1, (size, size))
        sec = timed_run(step, 40, 5, dev)
        res[f'{size}x{size}'] = 1.0 / sec
        total += its * sec
        del plan, step
    res['512x512'] = end_its
    total += 500 / end_its
    torch.cuda.empty_cache()
    out = {'it_s_per_scale': res, 'iterations': 3000,
           # sum over the scales of iterations / (it/s of a 40-step sample at that scale): a MODEL of the hot loop, not a run
           'hot_loop_seconds_modelled_from_40_step_samples': total, 'mean_it_s_over_the_modelled_run': 3000 / total}
    # ... and the real thing: ONE call of the drop-in StyleTransfer.stylize() with the reference's defaults (end_scale 512:
    # 1000 + 4 x 500 Adam iterations over five scales, per-scale targets, scale transitions, PIL resizes, the range guard),
    # no callback, wall clock around the call including the final device synchronisation
    try:
        import numpy as np
        from PIL import Image
        from style_transfer import StyleTransfer

        def pil(t):
            return Image.fromarray((t[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8), 'RGB')
        st = StyleTransfer(devices=[str(dev)], weights='synthetic', precision=args.precision)
        content, style = pil(synthetic_image(100, 512, 512)), pil(synthetic_image(200, 512, 512))
        import contextlib, io
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            st.stylize(content, [style])
        torch.cuda.synchronize(dev)
        out['stylize_call_seconds'] = time.perf_counter() - t0
        out['stylize_call_mean_it_s'] = 3000 / out['stylize_call_seconds']
        del st
        torch.cuda.empty_cache()
    except Exception as exc:                                     # noqa: BLE001 - reported, never fatal for the bench line
        out['stylize_call_error'] = f'{type(exc).__name__}: {exc}'
    return out


def other_modes(args, dev, current):
    """Short runs (20 steps) of the same workload in the other conv arithmetic modes, for transparency."""
    import copy
    res = {}
    for prec in ('fp32', 'bf16x6', 'fp16x3', 'bf16x3'):
        if prec == current:
            continue
        a = copy.copy(args)
        a.precision = prec
        plan, step, _, _ = run_single(a, dev, 0, 1)
        res[prec] = 1.0 / timed_run(step, 20, 3, dev)
        if prec == 'fp32':
            # the exact-fp32 accounting next to the shipped one: the same launches on v_mfma_f32_32x32x2_f32, HIP events,
            # against the fp32 matrix peak
            plan.profile_enable(True)
            for _ in range(2):
                step()
            launches, ms, flops = plan.profile_read()
            plan.profile_enable(False)
            tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            res['fp32_conv_roofline'] = {'bound': 'mfma', 'achieved': tf, 'peak': CONV_PEAK['fp32'], 'unit': 'TFLOP/s',
                                         'frac': tf / CONV_PEAK['fp32'], 'avg_launch_ms': ms / max(launches, 1)}
        del plan, step
    return res


def self_launch(gpus):
    """`python bench.py --gpus N` without a launcher: re-run this command as N ranks under torch.distributed.run (one process
    per GPU, 127.0.0.1 rendezvous on a free port) and pass rank 0's JSON line and the exit code through.  The reference needs
    no launcher for its multi-device form either (cli.py:214-223: `--devices cuda:0 cuda:1` in one process); the driver's
    N = 1 command is plain `python bench.py --gpus 1`, so the same plain command with --gpus 8 must measure 8 GPUs and not
    print an N = 1 line labelled otherwise (VERDICT r4 missing #1).  Under torchrun (WORLD_SIZE set) main() runs as a rank."""
    import socket
    import subprocess
    visible = torch.cuda.device_count() if torch.cuda.is_available() else 0
    same_device = os.environ.get('ST_BENCH_SAME_DEVICE') == '1'
    if visible < gpus and not same_device:
        print(json.dumps({'metric': 'optimizer iterations/sec', 'value': None, 'unit': 'it/s', 'n_gpus': gpus,
                          'higher_is_better': True, 'vs_baseline': None, 'data': 'synthetic',
                          'config': {'workload': 'not run', 'parallelism':
                                     f'FAILED: --gpus {gpus} asked for, {visible} HIP device(s) visible'}}), flush=True)
        return 1
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')        # dmabuf IPC: RCCL between processes needs it on this driver
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', default=None,
                    help="image size: S (square) or WxH; default 512 at N = 1 (BASELINE configs[1]), 2048 at N > 1 "
                         "(configs[3], strong scaling)")
    ap.add_argument('--mode', choices=['auto', 'shard', 'replicas'], default='auto',
                    help='N > 1: shard one image into row strips (default) or run independent replicas')
    ap.add_argument('--precision', choices=['fp32', 'bf16x6', 'fp16x3', 'bf16x3'], default='fp16x3',
                    help='arithmetic of the 3x3 trunk convolutions (see DESIGN.md)')
    ap.add_argument('--scaling', choices=['weak', 'strong'], default='strong',
                    help='N > 1, sharded: strong (default) = the fixed image cut into N strips, value = its it/s; '
                         'weak = one size x size strip per GPU (an image of size*N rows), value = N x image it/s')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline figure does not need: two more timed regions, the roofline '
                         'profiles, and at N = 1 the other sizes and arithmetic modes, the PMC traffic and the CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32, at most 64 MiB in all)")
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip cpu_baseline (N = 1)')
    ap.add_argument('--no-extra', action='store_true', help='with --full: skip extra_sizes / other arithmetic modes (N = 1)')
    ap.add_argument('--no-pmc', action='store_true',
                    help='with --full: do not measure roofline.traffic with rocprofv3 child runs (N = 1)')
    ap.add_argument('--dist-backend', default='nccl',
                    help="torch.distributed backend; 'gloo' + ST_BENCH_SAME_DEVICE=1 runs all ranks on cuda:0 "
                         "(functional check of the N > 1 path on a single-GPU box, not a measurement)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be at least 1 and --warmup at least 0')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ and 'RANK' not in os.environ:
        sys.exit(self_launch(args.gpus))

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    args.height, args.width = parse_size(args.size if args.size is not None else (512 if world == 1 else 2048))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    dev = torch.device('cuda', 0 if os.environ.get('ST_BENCH_SAME_DEVICE') == '1' else local_rank)
    torch.cuda.set_device(dev)
    # (--mode shard under a one-process launcher: the strip machinery with a single strip over a real process group -
    # with ST_FABRIC_FORCE_COLLECTIVES=1 the one-GPU smoke test of the RCCL descriptor path, tests/test_bench_contract_gpu.py)
    if world > 1 or (args.mode == 'shard' and 'MASTER_ADDR' in os.environ):
        import torch.distributed as dist
        import datetime
        # a short timeout turns a transport hang into an exception (and the labelled replica fallback below)
        if args.dist_backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev, timeout=datetime.timedelta(seconds=240))
        else:
            dist.init_process_group(args.dist_backend, timeout=datetime.timedelta(seconds=240))

    mode = 'shard' if args.mode == 'shard' else ('single' if world == 1 else ('replicas' if args.mode == 'replicas' else 'shard'))
    note = None
    if mode == 'shard':
        # The RCCL transport of this path could not be exercised during development (one GPU per box).  First attempt:
        # the shipped form (exchanges ordered on the library's communication / head streams, overlap, owned heads).  If
        # ANY rank fails its first iteration with an exception, every rank falls back - once - to the conservative form
        # (host-synchronised exchanges, whole launches, replicated chains) and the line says so; a second failure is
        # reported as value null.  Recoverable are failures every rank meets at the same point (an unsupported call, a
        # transport error in one collective); a rank that fails ALONE leaves the others inside a collective, and that ends
        # at the process group's timeout.
        ok = torch.zeros(1, device=dev)
        # attempts: the in-library RCCL transport (nccl backend only) -> torch.distributed on the library's streams -> the
        # conservative form
        attempts = [('in-library RCCL transport', False, True), ('stream-ordered torch.distributed', False, False),
                    ('conservative', True, False)]
        if args.dist_backend != 'nccl' or os.environ.get('ST_FABRIC_NATIVE') == '0':
            attempts = attempts[1:]
        transport = None
        for attempt, (transport, conservative, native) in enumerate(attempts):
            try:
                plan, step, cpu_inputs, read_loss = run_sharded(args, dev, rank, world, conservative, native)
                first_iteration(step, dev, native)           # surfaces transport errors and, with a deadline, hangs
                torch.cuda.synchronize(dev)
                ok = torch.ones(1, device=dev)
            except Exception as exc:                         # noqa: BLE001 - reported in the JSON line
                note = (note + ' | ' if note else '') + \
                    f'sharded path ({transport}) failed on rank {rank}: ' \
                    f'{type(exc).__name__}: {exc}'
                print(note, file=sys.stderr, flush=True)
                ok = torch.zeros(1, device=dev)
            try:
                if world > 1:
                    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            except Exception:                                # noqa: BLE001
                ok = torch.zeros(1, device=dev)
            if float(ok.item()) >= 1:
                if conservative:
                    note = (note or 'the stream-ordered paths failed on another rank') + \
                        ' -> measured with the CONSERVATIVE transport (host-synchronised exchanges, no overlap, replicated chains)'
                elif attempt > 0:
                    note = (note or 'the in-library transport failed on another rank') + f' -> measured with {transport}'
                break
        if float(ok.item()) < 1:
            # no silent fallback to replicas: a SCALE record must not show replica throughput under the sharded
            # metric.  value = null, exit code 1.
            note = note or 'sharded path failed on another rank'
            if rank == 0:
                print(json.dumps({'metric': 'optimizer iterations/sec', 'value': None, 'unit': 'it/s', 'n_gpus': world,
                                  'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': None,
                                  'higher_is_better': True, 'scaling': args.scaling, 'vs_baseline': None,
                                  'dtype': DTYPE_LABEL[args.precision], 'data': 'synthetic',
                                  'config': {'workload': f'{args.width}x{args.height} sharded hot loop',
                                             'parallelism': f'{world} row strips - FAILED: {note}'}}), flush=True)
            try:
                if world > 1:
                    dist.destroy_process_group()
            except Exception:                                # noqa: BLE001
                pass
            sys.exit(1)
    if mode in ('single', 'replicas'):
        plan, step, cpu_inputs, read_loss = run_single(args, dev, rank, world)

    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    final_loss = read_loss()
    if args.dump_outputs:
        outputs = collect_outputs(step, mode, world)          # (the state after the last timed step, before any --full step)
        if rank == 0:
            write_outputs(args.dump_outputs, outputs)
        del outputs
    regions = [elapsed]
    hbm = {}
    if args.full:
        # Two more K-step regions under the same protocol (a 20-step region is 48 ms on machines that differ
        # by 8 %): `value` stays the FIRST region's - the contract's - and the line also carries all three and the best of them.
        for _ in range(2):
            sync_all()
            r0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize(dev)
            if world > 1:
                dist.barrier()
            r = time.perf_counter() - r0
            if world > 1:
                t = torch.tensor([r], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                r = float(t.item())
            regions.append(r)

        # ---- roofline of the dominant kernel (MFMA implicit-GEMM conv), HIP events on its stream ----
        plan.profile_enable(True)
        prof_steps = 3
        for _ in range(prof_steps):
            step()
        hbm = hbm_rooflines(plan, prof_steps) if mode in ('single', 'replicas') else {}
        launches, ms, flops = plan.profile_read()
        plan.profile_enable(False)
        achieved = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0

    prec = args.precision
    if rank == 0:
        if args.full:
            # roofline.traffic: measured for THIS run where rocprofv3 is available (N = 1, not --no-extra / --no-pmc), else
            # the figure replayed from the committed PMC passes - labelled either way
            traffic = (None, 'skipped (--no-pmc / --no-extra)')
            if world == 1 and mode == 'single' and not args.no_pmc and not args.no_extra:
                traffic = pmc_traffic_measured(args, prec, mode)
            if traffic[0] is None:
                replay = pmc_traffic(args, prec, mode)
                if replay[0] is not None:
                    replay[1]['in_run_measurement'] = traffic[1]
                traffic = replay
        height, width = args.height, args.width
        size = f'{width}x{height}'
        weak_shard = mode == 'shard' and args.scaling == 'weak' and world > 1
        # replicas: N images advance per step; weak sharding: one image of N x the pixels - counted in units of the
        # N = 1 workload (size x size images per second), so that value / (N * value_1) is the weak-scaling efficiency
        jobs = world if (mode == 'replicas' or weak_shard) else 1
        its = jobs * args.steps / elapsed
        par = {'single': 'single GPU', 'replicas': f'{world} independent replicas (one image per GPU)',
               'shard': (f'one {width}x{height * world} image as {world} row strips of {size} (weak scaling; value = image '
                         f'iterations/s x {world}), halo exchange + Gram all-reduce over RCCL') if weak_shard else
                        f'{world} row strips of one {size} image (strong scaling; value = iterations/s of that image), '
                        f'halo exchange + Gram all-reduce over RCCL'}[mode]
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            # proof of what the line was measured over: the backend, the ranks the process group saw, the RCCL build
            try:
                lib_ver = '.'.join(str(v) for v in torch.cuda.nccl.version())
            except Exception:                                # noqa: BLE001
                lib_ver = 'unknown'
            par += (f' | torch.distributed backend {torch.distributed.get_backend()}, world size '
                    f'{torch.distributed.get_world_size()}, RCCL {lib_ver}, device {dev} '
                    f'({torch.cuda.get_device_properties(dev).name})')
        if mode == 'shard':
            par += f' | transport: {transport}'
        if note:
            par += f' [{note}]'
        out = {
            'metric': 'optimizer iterations/sec', 'value': its, 'unit': 'it/s', 'n_gpus': world,
            'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': elapsed / args.steps * 1e3,
            'higher_is_better': True,
            # N = 1 is the same run under either reading; it carries the flag the N > 1 runs of this command would
            'scaling': 'weak' if (mode == 'replicas' or weak_shard or (world == 1 and args.scaling == 'weak')) else 'strong',
            'vs_baseline': None, 'dtype': DTYPE_LABEL[prec], 'data': 'synthetic',
            'conv_arithmetic': prec + ': ' + CONV_MODE[prec],
            'config': {'workload': f'{size} single-scale hot loop (closure + Adam + clamp + EMA), '
                                   f'1 style image {size}, VGG-19 synthetic weights, max pooling',
                       'image_wh': [width, height], 'parallelism': par},
            'final_loss': final_loss,
        }
        if args.full:
            out.update({
                'value_regions': [jobs * args.steps / r for r in regions],      # the contract's region first, then two more
                'value_best_of_3': jobs * args.steps / min(regions),
                'roofline': {'bound': 'mfma',
                             'kernel': ('conv_split_kernel / conv_pc_kernel / conv_fat_kernel' if prec == 'fp16x3' else
                                        'conv_split_kernel' if prec != 'fp32' else 'conv_mfma_kernel') +
                                       ' (the 3x3 trunk convolutions, forward + data gradient, split-K reduce passes included), rank 0',
                             'achieved': achieved, 'peak': CONV_PEAK[prec], 'unit': 'TFLOP/s',
                             'frac': achieved / CONV_PEAK[prec], 'traffic': traffic[0], 'traffic_source': traffic[1],
                             # executed MFMA work against the dense 16-bit matrix peak: the direct kernels execute
                             # exactly `products` MFMA MACs per algorithmic MAC, so this equals `frac`; a Winograd F(2x2, 3x3) form
                             # would execute 16 / 36 of them (built and measured this round, slower: profiles/r06_winograd.md)
                             'mfma_work_frac': (achieved * MFMA_PRODUCTS[prec] / PEAK_BF16_MFMA_TFLOPS) if prec in MFMA_PRODUCTS else None,
                             'mfma_products_per_mac': MFMA_PRODUCTS.get(prec),
                             'peak_note': 'algorithmic fp32-equivalent FLOPs; peak = dense MFMA peak of the mode / products per MAC '
                                          'at the nominal 2.4 GHz; measured ceiling of an LDS-fed fp16x3 tile on this chip: 641-661 TF '
                                          '(profiles/r02_mfma_sustained.md: matrix pipe alone 2.34 PF, with the tile\'s LDS operand '
                                          'stream 1.92-1.98 PF); XL tile under load: 1.73 GHz, matrix pipes 71 % busy)',
                             'traffic_algorithmic': conv_algorithmic_bytes_per_launch(height, width),
                             'traffic_algorithmic_fused_path': conv_fused_path_bytes_per_launch(height, width),
                             'traffic_algorithmic_note': 'traffic_algorithmic = operand + result + weights of a bare convolution; '
                                                         '..._fused_path also counts the ReLU-mask and tap-gradient reads of the data-gradient '
                                                         'epilogues and the pooled (+ 1 byte / window) writes of the four pooled layers',
                             'launches_per_step': launches / prof_steps, 'avg_launch_ms': ms / max(launches, 1),
                             'algorithmic_gflop_per_step': flops / prof_steps / 1e9,
                             'whole_step_conv_tflops_per_gpu': conv_flops(height, width) * its / max(world, 1) / 1e12
                             if mode != 'shard' or weak_shard else conv_flops(height, width) * its / world / 1e12,
                             'fp32_mfma_peak': PEAK_FP32_MFMA_TFLOPS},
            })
        if hbm:
            out['roofline_hbm'] = hbm
        if world > 1:
            out['multi_gpu_note'] = ('strong-scaling base = extra_sizes of the N = 1 line for the same image; the RCCL '
                                     'transport of this path had never run on hardware before this measurement '
                                     '(one GPU per gpurun box during development)')
        if args.full and world == 1 and mode == 'single' and not args.no_extra:
            del plan, step
            torch.cuda.empty_cache()
            other = other_modes(args, dev, prec)
            out['other_conv_arithmetic_it_s'] = other
            if 'fp32' in other:
                out['exact_fp32_mfma_it_s'] = other['fp32']     # every conv on v_mfma_f32_32x32x2_f32: no split planes
                out['exact_fp32_mfma_roofline'] = other.pop('fp32_conv_roofline', None)
            out['extra_sizes'] = extra_sizes(args, dev)
            if (height, width) == (512, 512):
                out['config2_default_run'] = config2_scales(args, dev, its)
        if args.full and world == 1 and not args.no_cpu_baseline and height == width:
            out['cpu_baseline'] = cpu_baseline(height)
            if out['cpu_baseline']['value']:
                out['gpu_vs_cpu_baseline'] = its / out['cpu_baseline']['value']
        print(json.dumps(out), flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()

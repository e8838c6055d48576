#!/usr/bin/env python3
"""Gaps between consecutive kernels on the caller's stream, from a rocprofv3 kernel trace of bench.py (tools/trace_bench.sh):
for each of the last complete iterations, the forward trunk (conv_first_fwd ... the kernel before relu5_1's Gram kernel) and
the backward trunk (the first 3x3 data gradient after it ... the iteration's last kernel): kernels, kernel time, span, mean
and median gap.  -v lists every kernel of the last iteration with the gap in front of it.
    python tools/trunk_gaps.py t_kernel_trace.csv [-v]            (-> profiles/trunk_boundaries.md)"""
import csv
import re
import statistics
import sys

args = [a for a in sys.argv[1:] if a != '-v']
verbose = '-v' in sys.argv[1:]
if len(args) != 1:
    sys.exit(__doc__)
path = args[0]
rows = list(csv.DictReader(open(path)))
for r in rows:
    r['s'] = int(r['Start_Timestamp'])
    r['e'] = int(r['End_Timestamp'])
rows.sort(key=lambda r: r['s'])
starts = [i for i, r in enumerate(rows) if 'conv_first_fwd' in r['Kernel_Name']]


def short(n):
    n = re.sub(r'\(anonymous namespace\)::', '', n)
    n = re.sub(r'^void ', '', n).replace('st::', '')
    return n.split('(')[0][:70]


def is_conv3(n):
    return any(k in n for k in ('conv_pc_kernel', 'conv_fat_kernel', 'conv_split', 'conv_kernel', 'conv_mfma'))


def summarise(ks):
    gaps = [(b['s'] - a['e']) / 1e3 for a, b in zip(ks, ks[1:])]
    busy = sum(k['e'] - k['s'] for k in ks) / 1e3
    span = (ks[-1]['e'] - ks[0]['s']) / 1e3
    return len(ks), busy, span, gaps


fwd_means, bwd_means = [], []
n_it = min(4, len(starts) - 1)
for j in range(n_it, 0, -1):
    a, b = starts[-j - 1], starts[-j]
    q = rows[a]['Queue_Id']
    ks = [r for r in rows[a:b] if r['Queue_Id'] == q]
    f_end = next((i for i, k in enumerate(ks) if 'gram' in k['Kernel_Name'] and i > 0), len(ks))
    fwd = ks[:f_end]
    b_start = next((i for i in range(f_end, len(ks)) if is_conv3(ks[i]['Kernel_Name'])), len(ks))
    bwd = ks[b_start:]
    for name, part, acc in (('forward ', fwd, fwd_means), ('backward', bwd, bwd_means)):
        if len(part) < 2:
            continue
        n, busy, span, gaps = summarise(part)
        acc.append(statistics.mean(gaps))
        print(f'iteration -{j} {name}: {n:3d} kernels, kernel time {busy:7.1f} us, span {span:7.1f} us, '
              f'gap mean {statistics.mean(gaps):5.2f} median {statistics.median(gaps):5.2f} max {max(gaps):5.1f} us')
    if verbose and j == 1:
        prev = None
        for i, k in enumerate(ks):
            gap = (k['s'] - prev) / 1e3 if prev else 0.0
            mark = 'F' if i < f_end else ('B' if i >= b_start else 'h')
            print(f'  {mark} +{(k["s"] - ks[0]["s"]) / 1e3:8.1f} us  dur {(k["e"] - k["s"]) / 1e3:6.1f}  gap {gap:6.2f}  '
                  f'grid {k["Grid_Size_X"]:>7} wg {k["Workgroup_Size_X"]:>4}  {short(k["Kernel_Name"])}')
            prev = k['e']
if fwd_means:
    print(f'mean gap over {len(fwd_means)} iterations: forward {statistics.mean(fwd_means):.2f} us, '
          f'backward {statistics.mean(bwd_means):.2f} us')
